"""The detection loss without a GPU: invariants of the CPU restatement (tests/loss_util.py), the label buffer
(``preprocess``), the guards -- raised before any device is selected --, the loss session's launch plan on the meta
device and the C-ABI of ydbl_detect_loss (exports, descriptor layout against gcc, argument validation)."""

import ctypes as C
import subprocess
from pathlib import Path

import pytest
import torch

from loss_util import flatten_levels, reference_loss, rel_dist, synthetic_case

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ydbl.h"


@pytest.fixture(scope="module")
def yolo():
    from ydbl import YOLO

    return YOLO("yolov13n_DBL.yaml", nc=3)


@pytest.fixture(scope="module")
def base():
    levels, shapes, strides, gt = synthetic_case(0)
    box, cls = flatten_levels(levels)
    return box, cls, shapes, strides, gt, reference_loss(box, cls, shapes, strides, gt, dtype=torch.float64)


# ---------------------------------------------------------------------------------- invariants of the restatement
def test_image_without_labels_is_bce_only(base):
    box, cls, shapes, strides, gt, r = base
    assert not bool(r["fg"][2].any())
    assert float(r["per_image"][2, 0]) == 0.0 and float(r["per_image"][2, 2]) == 0.0
    bce0 = torch.nn.functional.softplus(cls[2].double()).sum() / r["target_scores_sum"] * 0.5
    assert rel_dist(r["per_image"][2, 1], bce0) < 1e-12
    # and a batch without any label: box and dfl stay 0, the normaliser is max(0, 1) = 1
    e = reference_loss(box, cls, shapes, strides, torch.zeros_like(gt), dtype=torch.float64)
    assert float(e["loss"][0]) == 0.0 and float(e["loss"][2]) == 0.0 and float(e["target_scores_sum"]) == 1.0
    assert rel_dist(e["loss"][1], torch.nn.functional.softplus(cls.double()).sum() * 0.5) < 1e-12


def test_duplicate_labels_give_the_lower_index_every_anchor(base):
    box, cls, shapes, strides, gt, _ = base
    g = gt.clone()
    g[1, 1] = g[1, 0]
    r = reference_loss(box, cls, shapes, strides, g, dtype=torch.float64)
    assert int((r["fg"][1] & (r["target_gt_idx"][1] == 0)).sum()) > 0
    assert int((r["fg"][1] & (r["target_gt_idx"][1] == 1)).sum()) == 0
    assert r["multi_selected"] >= 10  # every pick of the pair was a double pick


def test_label_without_an_anchor_centre_yields_no_fg(base):
    box, cls, shapes, strides, gt, _ = base
    g = torch.zeros_like(gt)
    g[0, 0] = torch.tensor([1.0, 1.0, 1.0, 3.0, 3.0])  # centres sit at multiples of 4 px: none inside
    r = reference_loss(box, cls, shapes, strides, g, dtype=torch.float64)
    assert r["in_box"] == [0] and not bool(r["fg"].any())
    assert float(r["loss"][0]) == 0.0 and float(r["loss"][2]) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_per_image_rows_sum_to_the_total(base, dtype):
    box, cls, shapes, strides, gt, _ = base
    r = reference_loss(box, cls, shapes, strides, gt, dtype=dtype)
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    for j in range(3):
        assert rel_dist(r["per_image"][:, j].sum(), r["loss"][j]) < tol
    assert 40 <= int(r["fg"].sum()) <= 70 and r["multi_selected"] >= 1 and r["short_labels"] >= 1


# ---------------------------------------------------------------------------------- preprocess
def test_pad_targets_hand_built():
    from ydbl.utils.loss import pad_targets

    # labels arrive in mixed image order; image 1 has none; xywh normalised of a 96 x 64 (w x h) input
    bidx = torch.tensor([2, 0, 2, 0, 0])
    cls = torch.tensor([[1.0], [0.0], [2.0], [1.0], [2.0]])  # [N, 1], as the reference's batches carry it
    xywh = torch.tensor([[0.5, 0.5, 0.25, 0.5], [0.25, 0.25, 0.5, 0.5], [0.75, 0.5, 0.125, 0.25],
                         [0.5, 0.75, 1 / 3, 0.125], [0.125, 0.125, 0.25, 0.25]])
    gt = pad_targets(bidx, cls, xywh, 3, (96, 64, 96, 64), max_labels=4, nc=3)
    assert gt.shape == (3, 4, 5) and gt.dtype == torch.float32
    want0 = torch.tensor([[0, 0.0, 0.0, 48.0, 32.0], [1, 32.0, 44.0, 64.0, 52.0], [2, 0.0, 0.0, 24.0, 16.0],
                          [0, 0, 0, 0, 0]])
    assert torch.allclose(gt[0], want0, atol=1e-5)
    assert torch.equal(gt[1], torch.zeros(4, 5))
    want2 = torch.tensor([[1, 36.0, 16.0, 60.0, 48.0], [2, 66.0, 24.0, 78.0, 40.0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
    assert torch.allclose(gt[2], want2, atol=1e-5)
    # the reference's preprocess on the same targets (loss.py:180-195), cut to its counts.max() rows
    t = torch.cat((bidx.view(-1, 1).float(), cls.view(-1, 1), xywh), 1)
    out = torch.zeros(3, 3, 5)
    for j in range(3):
        m = t[:, 0] == j
        if m.sum():
            out[j, : int(m.sum())] = t[m, 1:]
    b = out[..., 1:5] * torch.tensor([96.0, 64.0, 96.0, 64.0])
    out[..., 1:5] = torch.cat((b[..., :2] - b[..., 2:] / 2, b[..., :2] + b[..., 2:] / 2), -1)
    assert torch.equal(gt[:, :3], out)
    # xyxy pixels pass through; no labels at all is all padding
    px = pad_targets([1], [2.0], [[1.0, 2.0, 30.0, 40.0]], 2, None, max_labels=2, xywh=False, nc=3)
    assert px[1, 0].tolist() == [2.0, 1.0, 2.0, 30.0, 40.0] and float(px.abs().sum()) == 75.0
    assert float(pad_targets([], [], torch.zeros(0, 4), 2, (8, 8, 8, 8), max_labels=2, nc=3).abs().sum()) == 0.0


def test_gains_default_and_from_args(yolo):
    from types import SimpleNamespace

    from ydbl.utils.loss import loss_gains

    assert loss_gains(yolo.model) == (7.5, 0.5, 1.5)
    assert loss_gains(SimpleNamespace(args={"box": 1.0, "dfl": 2.0})) == (1.0, 0.5, 2.0)
    assert loss_gains(SimpleNamespace(args=SimpleNamespace(box=3.0, cls=4.0, dfl=5.0))) == (3.0, 4.0, 5.0)


# ---------------------------------------------------------------------------------- guards
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to pick a device fails the test: the guards must fire first."""
    import ydbl.engine.model as em
    import ydbl.engine.validator as ev

    def boom(*a, **k):
        raise AssertionError("a device was selected before the loss guards ran")

    monkeypatch.setattr(em, "select_device", boom)
    monkeypatch.setattr(ev, "select_device", boom)


def _batch(n_labels=2, cls=0.0, b=2):
    return {"img": torch.zeros(b, 3, 64, 96), "batch_idx": torch.zeros(n_labels),
            "cls": torch.full((n_labels, 1), cls), "bboxes": torch.full((n_labels, 4), 0.5)}


def test_label_guards_fire_on_the_host(yolo, no_device):
    m = yolo.model
    with pytest.raises(ValueError, match="max_labels=300"):
        m.loss(_batch(301))  # CPU img: the guard comes before the device check
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        m.loss(_batch(2, cls=3.0))
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        m(_batch(2, cls=-1.0))  # forward(dict) -> loss
    with pytest.raises(ValueError, match="batch_idx"):
        m.loss({**_batch(2), "batch_idx": torch.tensor([0.0, 2.0])})
    with pytest.raises(RuntimeError, match="MI355X"):  # valid labels: only now the device matters
        m.loss(_batch(300))
    crit = m.init_criterion()
    feats = [torch.zeros(2, 67, 8, 12), torch.zeros(2, 67, 4, 6), torch.zeros(2, 67, 2, 3)]
    with pytest.raises(ValueError, match="max_labels=300"):
        crit(feats, _batch(301))
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        crit((None, feats), _batch(1, cls=7.0))
    with pytest.raises(RuntimeError, match="MI355X"):
        crit(feats, _batch(1))


def test_val_guards_fire_before_device_selection(yolo, no_device):
    from ydbl.parallel import ShardedPredictor

    with pytest.raises(ValueError, match="augment"):
        yolo.val(data=[_batch()], loss=True, augment=True)
    with pytest.raises(ValueError, match="augment"):
        yolo.session(2, 64, 96, loss=True, augment=True)
    with pytest.raises(NotImplementedError, match="batch-sharded"):
        ShardedPredictor(yolo, 4, 64, 96, device=0, loss=True)
    with pytest.raises(NotImplementedError, match="batch-sharded"):
        yolo.session(2, 64, 96, loss=True, gather_rows=2)


# ---------------------------------------------------------------------------------- the plan (meta device)
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_loss_plan_on_meta(yolo, dtype):
    from ydbl.engine.session import DetectSession

    s = DetectSession(yolo.model, 2, 96, 128, dtype, conf=0.25, device="meta", streams=2, loss={"max_labels": 8})
    names = [st.fn.__name__ for st in s.plan.steps]
    whats = [st.what for st in s.plan.steps]
    assert names.count("ydbl_detect_loss") == 1 and names[-1] == "ydbl_detect_loss" and whats[-1] == "Detect.loss"
    last_head = max(i for i, w in enumerate(whats) if w.startswith("Detect.box") or "Conv1x1" in w)
    assert names.index("ydbl_detect_loss") > last_head
    assert not s.children and len(s.plans) == 1  # one plan whatever streams= says: one normaliser for the batch
    assert not s.sparse_box
    for st in s.plan.steps:  # no launch runs in the sparse box mode
        if st.fn.__name__ in ("ydbl_dsconv_nhwc", "ydbl_bottleneck_nhwc"):
            assert not st.args[0].tile_mask
    d = s.loss.desc
    assert (d.nl, d.nc, d.reg_max, d.max_labels, d.topk) == (3, 3, 16, 8, 10)
    assert [d.stride[i] for i in range(3)] == [8.0, 16.0, 32.0]
    assert (d.gain_box, d.gain_cls, d.gain_dfl) == (7.5, 0.5, 1.5)
    assert [(d.box[i].h, d.box[i].w, d.box[i].c, d.cls[i].c) for i in range(3)] == [(12, 16, 64, 3), (6, 8, 64, 3),
                                                                                    (3, 4, 64, 3)]
    assert tuple(s.loss.gt.shape) == (2, 8, 5) and tuple(s.loss.per_image.shape) == (2, 3)
    # without loss= nothing of it exists
    p = DetectSession(yolo.model, 2, 96, 128, dtype, conf=0.25, device="meta")
    assert p.loss is None and "ydbl_detect_loss" not in [st.fn.__name__ for st in p.plan.steps]


# ---------------------------------------------------------------------------------- C ABI
def test_loss_desc_layout_matches_c(tmp_path):
    from ydbl import _lib

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ydbl_loss_desc));']
    for fname, _ in _lib.LossDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(ydbl_loss_desc, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.splitlines() if line.strip())
    assert int(got["size"]) == C.sizeof(_lib.LossDesc)
    for fname, _ in _lib.LossDesc._fields_:
        assert int(got[fname]) == getattr(_lib.LossDesc, fname).offset, fname


def test_loss_validation_errors_without_gpu():
    from ydbl import _lib

    lib = _lib.lib
    assert lib.ydbl_detect_loss(None, None) == 1
    assert "null descriptor" in lib.ydbl_last_error().decode()
    d = _lib.LossDesc()
    d.nl, d.nc, d.reg_max, d.topk = 3, 3, 8, 10
    assert lib.ydbl_detect_loss(d, None) == 1 and "reg_max" in lib.ydbl_last_error().decode()
    d.reg_max, d.topk = 16, 17
    assert lib.ydbl_detect_loss(d, None) == 1 and "topk" in lib.ydbl_last_error().decode()
    d.topk = 10
    assert lib.ydbl_detect_loss(d, None) == 1 and "null buffer" in lib.ydbl_last_error().decode()
    assert lib.ydbl_detect_loss_workspace(0, 10, 1) == -1
    assert lib.ydbl_detect_loss_workspace(2, 126, -1) == -1
    # 8 words per anchor, 2 per label, 4 per 256-anchor block and 1 per image, each array rounded up to 16 bytes
    assert lib.ydbl_detect_loss_workspace(2, 126, 6) == 4 * (1008 + 4 * 252 + 2 * 12 + 8 + 4)
