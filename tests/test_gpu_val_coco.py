"""val(coco_eval=True) on the GPU (DBL-n, synthetic weights): metrics.coco_stats / coco_eval against the numpy
restatement of the COCO protocol (cocoeval_util.py) run on the very tensors the validator handed to coco_batch —
exact to 1e-12 and independent of the network's rounding —, for tensor batches, a dataset-backed run in native space
(coco_stats.csv, coco_summary()), single_cls / half / augment / fp8, and the default (nothing new runs)."""

import numpy as np
import pytest
import torch

import cocoeval_util as U
from confusion_util import pseudo_labels
from dataset_util import make_dataset

pytestmark = pytest.mark.gpu

TOL = 1e-12  # values in [0, 1], both sides fp64 sums of at most a few thousand terms
CONF = 0.05  # the synthetic weights score few boxes above 0.25 at these sizes; 0.05 keeps dozens per image


@pytest.fixture(scope="module")
def model(golden_dir):
    from parity_util import build_pair

    return build_pair("n", 3, golden_dir)[0]


@pytest.fixture
def recorded(monkeypatch):
    """Every coco_batch call of the validator: its detections read back, and the labels as passed."""
    from ydbl.engine import validator

    calls, real = [], validator.coco_batch

    def spy(det, count, gt_box, gt_cls, batch_idx, nc, single_cls=False, grouped=None, **kw):
        assert not kw  # the validator runs the protocol's own thresholds, ranges and cut
        calls.append(((det.float().cpu().numpy().copy(), count.cpu().numpy().copy(), gt_box.numpy().copy(),
                       gt_cls.numpy().copy(), batch_idx.numpy().copy()), nc, bool(single_cls)))
        return real(det, count, gt_box, gt_cls, batch_idx, nc, single_cls, grouped=grouped)

    monkeypatch.setattr(validator, "coco_batch", spy)
    return calls


@pytest.fixture(scope="module")
def tensor_batches(model):
    """Two in-memory batches of four 128 x 128 images, labelled from the model's own detections."""
    from ydbl.engine import validator
    from ydbl.utils.synthetic import blob_images

    x = blob_images(8, 128, seed=77)
    seen, real = [], validator.confusion_batch
    validator.confusion_batch = lambda det, count, *a, **k: seen.append((det.cpu().clone(), count.cpu().clone()))
    try:
        dummy = {"cls": torch.zeros(1), "bboxes": torch.tensor([[0.0, 0.0, 5.0, 5.0]]), "batch_idx": torch.zeros(1)}
        model.val(data=[{"img": x[:4], **dummy}, {"img": x[4:], **dummy}])
    finally:
        validator.confusion_batch = real
    batches = []
    for k, (det, cnt) in enumerate(seen):
        boxes, cls, bidx = pseudo_labels(det, cnt, 128, cut=CONF)
        batches.append({"img": x[4 * k: 4 * k + 4], "cls": cls, "bboxes": boxes, "batch_idx": bidx})
    return batches


def check_against_restatement(m, calls, nc):
    """metrics.coco_stats / coco_eval equal the restatement on the recorded calls; returns the stats."""
    assert len({(c[1], c[2]) for c in calls}) == 1 and calls[0][1] == nc
    _, _, ev, stats = U.run([c[0] for c in calls], nc, calls[0][2])
    got = m.coco_stats
    print("coco stats:", dict(zip(m.coco_stat_names, np.round(got, 6))))
    assert got.dtype == np.float64 and got.shape == (12,) and np.abs(got - stats).max() <= TOL
    assert m.coco_stat_names == U.STAT_NAMES
    e = m.coco_eval
    assert set(e) >= {"precision", "recall", "scores", "params", "counts"} and e["counts"] == [10, 101, nc, 4, 3]
    assert e["precision"].shape == (10, 101, nc, 4, 3) and e["recall"].shape == (10, nc, 4, 3)
    for key in ("precision", "recall", "scores"):
        assert np.abs(e[key] - ev[key]).max() <= TOL, key
    assert np.array_equal(e["params"]["iouThrs"], U.IOU_THRS) and e["params"]["maxDets"] == U.MAX_DETS
    # the protocol's own invariants
    assert got[6] <= got[7] <= got[8] and got[2] <= got[1]
    p = e["precision"][:, :, :, 0, 2]
    per_t = [p[t][p[t] > -1].mean() for t in range(10)]
    assert abs(got[0] - np.mean(per_t)) <= TOL and abs(got[1] - per_t[0]) <= TOL and abs(got[2] - per_t[5]) <= TOL
    return got


def test_val_coco_tensor_batches(model, tensor_batches, recorded):
    m = model.val(data=tensor_batches, conf=CONF, coco_eval=True)
    assert len(recorded) == 2 and model.validator.seen == 8
    got = check_against_restatement(m, recorded, 3)
    assert got[0] > 0 and got[8] > 0  # the pseudo-labels are found
    lines = model.validator.coco_summary()
    assert len(lines) == 12 and lines[0].startswith(" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all |")
    assert lines[0].endswith("= %0.3f" % got[0]) and lines[8].endswith("maxDets=100 ] = %0.3f" % got[8])

    # the default: no call, no new field, the same numbers as without the argument — and as with coco_eval=True
    del recorded[:]
    m0 = model.val(data=tensor_batches, conf=CONF)
    m1 = model.val(data=tensor_batches, conf=CONF, coco_eval=False)
    assert not recorded
    for a in (m0, m1):
        assert a.coco_stats is None and a.coco_eval is None
        assert a.results_dict == m.results_dict and np.array_equal(a.box.all_ap, m.box.all_ap)
        assert np.array_equal(a.confusion_matrix.matrix, m.confusion_matrix.matrix)
    assert vars(m0).keys() == vars(m1).keys() and vars(m0.box).keys() == vars(m1.box).keys()
    assert model.validator.coco_batches == []
    with pytest.raises(RuntimeError):
        model.validator.coco_summary()


@pytest.mark.parametrize("kw", [{"single_cls": True}, {"half": True}, {"augment": True}, {"half": True, "fp8": True}],
                         ids=["single_cls", "half", "augment", "fp8"])
def test_val_coco_modes(model, tensor_batches, recorded, kw, capsys):
    m = model.val(data=tensor_batches, conf=CONF, coco_eval=True, verbose=True, **kw)
    assert len(recorded) == 2 and all(c[2] == bool(kw.get("single_cls")) for c in recorded)
    check_against_restatement(m, recorded, 3)
    out = capsys.readouterr().out
    assert out.count("Average Precision  (AP)") == 6 and out.count("Average Recall     (AR)") == 6
    assert out.index("mAP50-95)") < out.index("Average Precision")  # after the class table


def test_val_coco_dataset(model, tmp_path, recorded):
    y = make_dataset(tmp_path / "ds", shapes=[(120, 160), (160, 120), (90, 160), (125, 125)], edge_cases=False)
    out = tmp_path / "out"
    m = model.val(data=str(y), imgsz=160, batch=4, conf=CONF, coco_eval=True, save_dir=str(out))
    assert len(recorded) == 1 and model.validator.seen == 4
    (det, cnt, boxes, cls, bidx), nc, single = recorded[0]
    assert len(cls) > 0 and cnt.sum() > 0 and not single
    got = check_against_restatement(m, recorded, 3)
    rows = (out / "coco_stats.csv").read_text().splitlines()
    assert len(rows) == 2 and rows[0].split(",") == U.STAT_NAMES
    assert [float(v) for v in rows[1].split(",")] == got.tolist()
    lines = model.validator.coco_summary()
    assert [ln.split("=")[-1].strip() for ln in lines] == ["%0.3f" % v for v in got]
    assert sum("Average Recall" in ln for ln in lines) == 6

    # without save_dir nothing is written; the Ultralytics numbers do not depend on coco_eval
    before = sorted(f.name for f in tmp_path.rglob("*"))
    m2 = model.val(data=str(y), imgsz=160, batch=4, conf=CONF, coco_eval=True)
    assert sorted(f.name for f in tmp_path.rglob("*")) == before and np.array_equal(m2.coco_stats, got)
    m3 = model.val(data=str(y), imgsz=160, batch=4, conf=CONF)
    assert m3.results_dict == m.results_dict and m3.coco_stats is None
