"""The detection loss end to end on the GPU: DetectionModel.loss / forward(dict) as one captured graph, the criterion
on forward's outputs, val(loss=True) on tensor batches and on a dataset, the untouched default, and one fp8 run.
DBL-n nc=3 with the trained-like fixture at 128 x 128, batch 4 (A = 336: two workgroups per image).

The reference values come from the CPU restatement (tests/loss_util.py) applied to the very level maps the session
computed (feats()) and the very label buffer the kernel read; the tolerance is the kernel test's: 32 x the fp32
restatement's own relative distance to the fp64 one on these inputs (tests/test_gpu_loss.py).  The distance to the
same restatement on the CPU oracle model's levels -- other conv paths, possibly another assignment -- is printed as a
figure (profiles/r18/r18_loss_parity.txt), not asserted.
"""

import numpy as np
import pytest
import torch

from loss_util import GAINS, random_labels, reference_loss, rel_dist

pytestmark = pytest.mark.gpu

B, S, NC = 4, 128, 3
COUNTS = (5, 3, 0, 2)
FACTOR = 32.0
KEYS = ["val/box_loss", "val/cls_loss", "val/dfl_loss"]


def table_dist(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1, 3), torch.as_tensor(b).double().reshape(-1, 3)
    return max(rel_dist(a[:, j], b[:, j]) for j in range(3))


def make_batch(seed, x):
    """A reference batch dict (normalised xywh) of random labels for the images x, and the same labels as xyxy
    pixels (what val()'s tensor batches carry)."""
    gen = torch.Generator().manual_seed(seed)
    gt = random_labels(gen, COUNTS, S, S, max(COUNTS), NC)
    rows = [(b, gt[b, m]) for b in range(B) for m in range(COUNTS[b])]
    bidx = torch.tensor([float(b) for b, _ in rows])
    cls = torch.stack([r[0] for _, r in rows]).view(-1, 1)
    xyxy = torch.stack([r[1:] for _, r in rows])
    xywh = torch.cat(((xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]), 1) / S
    return ({"img": x, "batch_idx": bidx, "cls": cls, "bboxes": xywh},
            {"img": x, "batch_idx": bidx, "cls": cls.view(-1), "bboxes": xyxy})


@pytest.fixture(scope="module")
def pair(golden_dir):
    from parity_util import build_pair

    return build_pair("n", NC, golden_dir)


@pytest.fixture(scope="module")
def data():
    from ydbl.utils.synthetic import blob_images

    x = blob_images(2 * B, S, seed=77)
    return [make_batch(11, x[:B]), make_batch(12, x[B:])]


def restate(feats, gt):
    """fp32 and fp64 restatements on NCHW level maps [B, 64+nc, h, w] and a padded label buffer."""
    feats = [f.detach().float().cpu() for f in feats]
    flat = torch.cat([f.flatten(2).permute(0, 2, 1) for f in feats], 1)
    shapes = [tuple(f.shape[2:]) for f in feats]
    box, cls = flat[..., :64].contiguous(), flat[..., 64:].contiguous()
    gt = gt.detach().float().cpu()
    r32 = reference_loss(box, cls, shapes, [8, 16, 32], gt, GAINS, torch.float32)
    r64 = reference_loss(box, cls, shapes, [8, 16, 32], gt, GAINS, torch.float64)
    assert torch.equal(r32["fg"], r64["fg"]) and torch.equal(r32["target_gt_idx"], r64["target_gt_idx"]), \
        "the inputs are not decidable in fp32"
    yard = max(table_dist(r32["loss"], r64["loss"]), table_dist(r32["per_image"], r64["per_image"]))
    return r64, yard


@pytest.mark.parametrize("half", [False, True])
def test_model_loss_in_graph(pair, data, half):
    p, o = pair
    dev = torch.device("cuda", 0)
    batch = dict(data[0][0])
    batch["img"] = batch["img"].to(dev).half() if half else batch["img"].to(dev)
    total, items = p.model.loss(batch)
    total2, items2 = p.model(batch)  # forward(dict) -> loss: the same graph replayed
    assert items.dtype == torch.float32 and items.device.type == "cuda" and tuple(items.shape) == (3,)
    assert torch.equal(items, items2) and torch.equal(total, total2)
    assert float(total) == pytest.approx(float(items.sum()) * B, rel=1e-6)
    s = p.model._forward_session(B, S, S, half, dev, loss=True)
    assert s.loss is not None and not s.sparse_box and not s.children
    assert [st.fn.__name__ for st in s.plan.steps].count("ydbl_detect_loss") == 1
    torch.cuda.synchronize()
    r, yard = restate(s.feats(), s.loss.gt)
    d_loss = table_dist(items.cpu(), r["loss"])
    d_img = table_dist(s.loss.per_image.cpu(), r["per_image"])
    print(f"model.loss {'fp16' if half else 'fp32'}: loss {[float(v) for v in items.cpu()]} fg {int(r['fg'].sum())} "
          f"multi {r['multi_selected']} min gap {min(r['gaps']):.3g} | yard {yard:.3g} d(loss) {d_loss:.3g} "
          f"d(per_image) {d_img:.3g}")
    assert int(r["fg"].sum()) > 0 and torch.isfinite(items).all()
    assert d_loss <= FACTOR * yard and d_img <= FACTOR * yard
    # figure only: the same restatement on the CPU oracle's levels (its own conv paths)
    with torch.no_grad():
        _, ofeats = o(data[0][0]["img"])
    ro = reference_loss(*_flat(ofeats), [8, 16, 32], s.loss.gt.cpu(), GAINS, torch.float64)
    print(f"model.loss {'fp16' if half else 'fp32'} vs the restatement on the CPU oracle's levels: d(loss) "
          f"{table_dist(items.cpu(), ro['loss']):.3g}, fg anchors that differ "
          f"{int((ro['fg'] != r['fg']).sum())} of {int(r['fg'].sum())}")


def _flat(feats):
    feats = [f.detach().double().cpu() for f in feats]
    flat = torch.cat([f.flatten(2).permute(0, 2, 1) for f in feats], 1)
    return flat[..., :64].contiguous(), flat[..., 64:].contiguous(), [tuple(f.shape[2:]) for f in feats]


@pytest.mark.parametrize("half", [False, True])
def test_criterion_on_forward_outputs(pair, data, half):
    p, _ = pair
    dev = torch.device("cuda", 0)
    batch = dict(data[0][0])
    x = batch["img"].to(dev).half() if half else batch["img"].to(dev)
    batch["img"] = x
    _, items = p.model.loss(batch)
    y, feats = p.model(x)
    crit = p.model.init_criterion()
    total, got = crit((y, feats), batch)
    _, got2 = p.model.loss(batch, preds=feats)
    torch.cuda.synchronize()
    r, yard = restate(feats, crit.preprocess(batch, B, (S, S)))
    print(f"criterion {'fp16' if half else 'fp32'}: {[float(v) for v in got.cpu()]} in-graph "
          f"{[float(v) for v in items.cpu()]} | yard {yard:.3g} d(restatement) {table_dist(got.cpu(), r['loss']):.3g} "
          f"d(in-graph) {table_dist(got.cpu(), items.cpu()):.3g}")
    assert torch.equal(got, got2)
    assert float(total) == pytest.approx(float(got.sum()) * B, rel=1e-6)
    assert table_dist(got.cpu(), r["loss"]) <= FACTOR * yard
    assert table_dist(crit.per_image.cpu(), r["per_image"]) <= FACTOR * yard
    assert table_dist(got.cpu(), items.cpu()) <= FACTOR * yard  # the in-graph path: the same levels, another plan


def _check_val(v, m, n_batches, n_images):
    assert tuple(v.batch_loss.shape) == (n_batches, 3) and tuple(v.image_loss.shape) == (n_images, 3)
    assert torch.allclose(torch.tensor(m.val_loss), v.batch_loss.sum(0) / n_batches, rtol=1e-6, atol=0)
    rd = m.results_dict
    assert [rd[k] for k in KEYS] == list(m.val_loss) and all(v_ > 0 for v_ in m.val_loss)
    assert (v.save_dir / "val_loss.csv").exists()
    rows = (v.save_dir / "val_loss.csv").read_text().strip().splitlines()
    assert rows[0] == "image,box_loss,cls_loss,dfl_loss" and rows[1].startswith("all,") and len(rows) == 2 + n_images


def test_val_loss_tensor_batches(pair, data, tmp_path):
    p, _ = pair
    batches = [d[1] for d in data]
    m = p.val(data=batches, loss=True, save_dir=tmp_path)
    v = p.validator
    _check_val(v, m, 2, 2 * B)
    for k in range(2):  # each batch's rows add up to that batch's values
        assert table_dist(v.image_loss[k * B:(k + 1) * B].double().sum(0), v.batch_loss[k]) <= 1e-6
    # a batch's values are what the model's own loss gives on the same labels (xyxy pixels here, xywh there: the
    # labels agree to an ulp or two of 128, the loss to a few 1e-6)
    _, items = p.model.loss({**data[0][0], "img": data[0][0]["img"].cuda()})
    print(f"val(loss=True): val_loss {m.val_loss} batch 0 {v.batch_loss[0].tolist()} model.loss "
          f"{items.cpu().tolist()} d {table_dist(v.batch_loss[0], items.cpu()):.3g}")
    assert table_dist(v.batch_loss[0], items.cpu()) <= 1e-4


def test_val_default_is_untouched(pair, data):
    p, _ = pair
    batches = [d[1] for d in data]
    m1 = p.val(data=batches, loss=True)
    assert hasattr(p.validator, "image_loss")
    keys1 = dict(m1.results_dict)
    m0 = p.val(data=batches)
    v0 = p.validator
    assert "val_loss" not in vars(m0) and not hasattr(m0, "val_loss")
    for name in ("image_loss", "batch_loss", "loss_batches", "loss_files"):
        assert not hasattr(v0, name), name
    assert list(m0.results_dict) == [*type(m0).keys, "fitness"]
    for k, val in m0.results_dict.items():  # every existing field keeps its value
        assert val == keys1[k], k
    assert np.array_equal(np.asarray(m0.box.all_ap), np.asarray(m1.box.all_ap))
    assert (m0.confusion_matrix.matrix == m1.confusion_matrix.matrix).all()
    for s in p._sessions.values():  # the default's session holds no loss step
        if getattr(s, "loss", None) is None:
            assert all(st.fn.__name__ != "ydbl_detect_loss" for pl in s.plans for st in pl.steps)


def test_val_loss_dataset(pair, tmp_path):
    from dataset_util import SHAPES, make_dataset

    p, _ = pair
    y = make_dataset(tmp_path / "ds", shapes=SHAPES[:6], edge_cases=False)
    m = p.val(data=str(y), imgsz=S, batch=B, loss=True, save_dir=tmp_path / "out", half=True)
    v = p.validator
    _check_val(v, m, 2, 6)
    assert table_dist(v.image_loss[:B].double().sum(0), v.batch_loss[0]) <= 1e-6
    assert table_dist(v.image_loss[B:].double().sum(0), v.batch_loss[1]) <= 1e-6
    names = [r.split(",")[0] for r in (tmp_path / "out" / "val_loss.csv").read_text().strip().splitlines()[2:]]
    assert names == v.loss_files and len(set(names)) == 6 and all(n.endswith(".png") for n in names)
    print(f"val(data=yaml, loss=True, half=True): val_loss {m.val_loss}")
    ms = p.val(data=str(y), imgsz=S, batch=B, loss=True, single_cls=True)
    assert all(torch.isfinite(torch.tensor(ms.val_loss)))


def test_val_loss_fp8(golden_dir, data):
    from parity_util import build_pair

    p, _ = build_pair("s", NC, golden_dir)
    m = p.val(data=[data[0][1]], loss=True, fp8=True, fp8_calibration=golden_dir / "fp8_calib_yolov13s_DBL_nc3.json")
    print(f"val(loss=True, fp8=True) DBL-s: val_loss {m.val_loss}")
    assert len(m.val_loss) == 3 and all(torch.isfinite(torch.tensor(m.val_loss))) and all(v > 0 for v in m.val_loss)
