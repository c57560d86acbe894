"""val()'s full report on the GPU (DBL-n, synthetic weights): metrics.confusion_matrix against the CPU restatement
of ConfusionMatrix.process_batch (confusion_util.py) applied to the very tensors the validator handed to the
kernel — exact, and independent of the network's rounding —, the per-class table, plots=False, and the
predictions.json / label files of dataset-backed runs (U/models/yolo/detect/val.py:125-201, :270-295)."""

import json

import numpy as np
import pytest
import torch

from confusion_util import confusion_reference, pseudo_labels
from dataset_util import make_dataset

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(golden_dir):
    from parity_util import build_pair

    return build_pair("n", 3, golden_dir)[0]


@pytest.fixture
def recorded(monkeypatch):
    """Every confusion_batch call of the validator: its detections read back, and the labels as passed."""
    from ydbl.engine import validator

    calls, real = [], validator.confusion_batch

    def spy(det, count, gt_box, gt_cls, batch_idx, cm, single_cls=False, grouped=None):
        calls.append((det.cpu().clone(), count.cpu().clone(), gt_box.clone(), gt_cls.clone(), batch_idx.clone(),
                      bool(single_cls)))
        return real(det, count, gt_box, gt_cls, batch_idx, cm, single_cls, grouped=grouped)

    monkeypatch.setattr(validator, "confusion_batch", spy)
    return calls


CONF = 0.05  # the synthetic weights score few boxes above 0.25 at these sizes; 0.05 keeps dozens per image


def _reference(calls, nc, conf):
    """The checker over the recorded calls.  A multi-label NMS keeps one box once per class, so these inputs carry
    exact IoU ties; kind="stable" is the reference's argsort with the order on ties that numpy only defines for
    up to 16 matches (confusion_util.process_batch), the rule the kernel documents."""
    total = np.zeros((nc + 1, nc + 1))
    for det, cnt, boxes, cls, bidx, single in calls:
        total += confusion_reference(det, cnt, boxes, cls, bidx, nc, conf=conf, single_cls=single, kind="stable")
    return total


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


def test_val_report_tensor_batches(model, tensor_batches, recorded):
    m = model.val(data=tensor_batches, conf=CONF)
    v = model.validator
    assert len(recorded) == 2 and v.seen == 8
    cm = m.confusion_matrix
    assert cm is v.confusion_matrix and cm.nc == 3 and cm.conf == CONF
    got = cm.matrix
    ref = _reference(recorded, 3, conf=CONF)
    print("confusion matrix (rows predicted, columns true, last = background):\n", got)
    assert got.dtype == np.float64 and np.array_equal(got, ref)
    assert np.trace(got[:3, :3]) > 0 and got[3, :3].sum() > 0 and got[:3, 3].sum() > 0
    # every label is counted once in its class's column
    n_labels = sum(len(b["cls"]) for b in tensor_batches)
    assert np.array_equal(got[:, :3].sum(0), v.nt_per_class) and v.nt_per_class.sum() == n_labels
    per_image = sum(len(torch.unique(b["cls"][b["batch_idx"] == i])) for b in tensor_batches for i in range(4))
    assert v.nt_per_image.sum() == per_image and (v.nt_per_image <= 8).all()
    # the per-class report is consistent with box.all_ap
    ap = m.box.all_ap
    assert len(m.ap_class_index) == ap.shape[0] > 0
    assert m.mean_results() == [m.box.mp, m.box.mr, ap[:, 0].mean(), ap[:, 5].mean(), ap.mean()]
    for i, c in enumerate(m.ap_class_index):
        assert m.class_result(i) == (m.box.p[i], m.box.r[i], ap[i, 0], ap[i, 5], ap[i].mean())
        assert m.maps[c] == ap[i].mean()
    assert m.maps.shape == (3,) and len(m.curves_results) == 4 and m.curves_results[1][1].shape == (ap.shape[0], 1000)
    lines = v.print_results()
    assert len(lines) == 1 + ap.shape[0] and lines[0].split()[:3] == ["all", "8", str(n_labels)]
    assert all(len(ln.split()) == 8 for ln in lines)
    c0 = int(m.ap_class_index[0])
    assert lines[1].split()[:3] == [model.names[c0], str(v.nt_per_image[c0]), str(v.nt_per_class[c0])]
    assert float(lines[0].split()[5]) == float("%.3g" % m.box.map50)

    # plots=False skips the accumulation and changes no metric; neither do the save arguments without save_dir
    m50, m5095, rd = m.box.map50, m.box.map, m.results_dict
    n_calls = len(recorded)
    m2 = model.val(data=tensor_batches, conf=CONF, plots=False)
    assert len(recorded) == n_calls and not m2.confusion_matrix.matrix.any()
    assert (m2.box.map50, m2.box.map) == (m50, m5095) and m2.results_dict == rd
    m3 = model.val(data=tensor_batches, conf=CONF, save_json=True, save_txt=True, save_conf=True, verbose=True)
    assert (m3.box.map50, m3.box.map) == (m50, m5095) and np.array_equal(m3.confusion_matrix.matrix, got)
    assert list(model.validator.stats) == ["tp", "conf", "pred_cls", "target_cls"]

    # val's own default: conf 0.001 for the NMS, 0.25 for the confusion matrix (:311)
    del recorded[:]
    m4 = model.val(data=tensor_batches)
    assert m4.confusion_matrix.conf == 0.25
    got4 = m4.confusion_matrix.matrix
    assert np.array_equal(got4, _reference(recorded, 3, conf=0.001))
    assert np.array_equal(got4[:, :3].sum(0), model.validator.nt_per_class) and got4.sum() < got.sum()


def test_val_report_dataset(model, tmp_path, recorded):
    y = make_dataset(tmp_path / "ds", shapes=[(120, 160), (160, 120), (90, 160), (125, 125)], edge_cases=False)
    out = tmp_path / "out"
    m = model.val(data=str(y), imgsz=160, batch=4, conf=CONF, save_json=True, save_txt=True, save_conf=True,
                  save_dir=str(out))
    v = model.validator
    assert len(recorded) == 1 and v.seen == 4
    det, cnt, boxes, cls, bidx, _ = recorded[0]
    got = m.confusion_matrix.matrix
    assert np.array_equal(got, _reference(recorded, 3, conf=CONF))
    assert np.array_equal(got[:, :3].sum(0), v.nt_per_class) and v.nt_per_class.sum() == len(cls) > 0
    assert got[:3].sum() > 0  # some detection passes the cut

    # predictions.json: one row per detection, in image order, from the native-space boxes the kernel saw
    rows = json.loads((out / "predictions.json").read_text())
    assert len(rows) == int(cnt.sum()) > 0
    from pathlib import Path

    stems = [Path(lb["im_file"]).stem for lb in v.dataset.labels]  # the rect order the batch was built in
    assert sorted(stems) == [f"im{i:03d}" for i in range(4)]
    k = 0
    for si, stem in enumerate(stems):
        p = det[si, : cnt[si]]
        wh = p[:, 2:4] - p[:, 0:2]
        tl = (p[:, 0:2] + p[:, 2:4]) / 2 - wh / 2  # xyxy2xywh, then centre -> top-left, in fp32 like the reference
        for j in range(len(p)):
            r = rows[k]
            assert set(r) == {"image_id", "category_id", "bbox", "score"} and r["image_id"] == stem
            assert r["category_id"] == int(p[j, 5]) + 1
            assert r["bbox"] == [round(t, 3) for t in (*tl[j].tolist(), *wh[j].tolist())]
            assert r["score"] == round(p[j, 4].item(), 5)
            k += 1
        # labels/<stem>.txt: 'cls xc yc w h conf', normalized by the original image
        txt = [ln.split() for ln in (out / "labels" / f"{stem}.txt").read_text().splitlines()]
        assert len(txt) == len(p) and all(len(t) == 6 for t in txt)
        h0, w0 = v.dataset.labels[si]["shape"]
        assert [int(t[0]) for t in txt] == p[:, 5].int().tolist()
        want = torch.stack([(p[:, 0] + p[:, 2]) / 2 / w0, (p[:, 1] + p[:, 3]) / 2 / h0, wh[:, 0] / w0, wh[:, 1] / h0,
                            p[:, 4]], 1)
        assert np.allclose(np.array([[float(s) for s in t[1:]] for t in txt]), want.numpy(), rtol=1e-5, atol=1e-6)
    assert k == len(rows)

    # without save_dir nothing is written, and the numbers do not move
    before = sorted(f.name for f in tmp_path.rglob("*"))
    m2 = model.val(data=str(y), imgsz=160, batch=4, conf=CONF, save_json=True, save_txt=True)
    assert sorted(f.name for f in tmp_path.rglob("*")) == before
    assert (m2.box.map50, m2.box.map) == (m.box.map50, m.box.map)
