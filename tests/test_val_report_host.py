"""The host side of val()'s full report: DetMetrics' per-class accessors and curves (U/utils/metrics.py:626-906 of
this fork, mAP75 as a fifth column), the predictions.json / label-file formatting (U/models/yolo/detect/val.py:
270-295) and ConfusionMatrix.tp_fp() / print() on a given matrix.  No GPU."""

import json
import logging

import numpy as np
import pytest
import torch


def _stats(seed=0, n=400, classes=(0, 2)):
    """Detections of classes 0 and 2 (class 1 has no labels, class 3 labels but no detections)."""
    rng = np.random.default_rng(seed)
    conf = rng.uniform(0.01, 1.0, n)
    pred_cls = rng.choice(classes, n).astype(np.float64)
    # a detection is more likely right when confident, and rarer at the stricter IoU thresholds
    tp = rng.uniform(0, 1, (n, 1)) < conf[:, None] * np.linspace(1.0, 0.3, 10)[None]
    tp = np.logical_and.accumulate(tp, 1)
    target_cls = np.concatenate([np.zeros(90), np.full(120, 2.0), np.full(7, 3.0)])
    return tp, conf, pred_cls, target_cls


def test_ap_per_class_curves_are_additional():
    from ydbl.utils.metrics import ap_per_class

    st = _stats()
    base = ap_per_class(*st)
    full = ap_per_class(*st, curves=True)
    assert len(base) == 7 and len(full) == 12
    for a, b in zip(base, full):
        assert np.array_equal(a, b)
    p_curve, r_curve, f1_curve, x, prec_values = full[7:]
    assert p_curve.shape == r_curve.shape == f1_curve.shape == (3, 1000) and x.shape == (1000,)
    assert prec_values.shape == (2, 1000)  # only classes with predictions and labels (:586-587, :605)
    assert np.array_equal(x, np.linspace(0, 1, 1000))
    assert np.allclose(f1_curve, 2 * p_curve * r_curve / (p_curve + r_curve + 1e-16))
    assert (np.diff(r_curve, axis=1) <= 1e-12).all()  # recall falls as the confidence cut rises
    assert (np.diff(prec_values, axis=1) <= 1e-12).all()  # the precision envelope is non-increasing over recall


def test_det_metrics_accessors():
    from ydbl.utils.metrics import DetMetrics, ap_per_class

    names = {0: "a", 1: "b", 2: "c", 3: "d", 4: "e"}
    m = DetMetrics(names=names)
    assert m.mean_results() == [0.0, 0.0, 0.0, 0.0, 0.0] and len(m.maps) == 0 and m.confusion_matrix is None
    st = _stats()
    m.process(*st)
    _, _, p, r, f1, ap, idx = ap_per_class(*st)
    b = m.box
    assert list(m.ap_class_index) == [0, 2, 3] and np.array_equal(b.all_ap, ap)
    assert np.array_equal(b.ap50, ap[:, 0]) and np.array_equal(b.ap75, ap[:, 5])
    assert np.array_equal(b.ap, ap.mean(1))
    assert m.mean_results() == [b.mp, b.mr, b.map50, b.map75, b.map]
    assert m.mean_results() == [p.mean(), r.mean(), ap[:, 0].mean(), ap[:, 5].mean(), ap.mean()]
    for i in range(3):
        assert m.class_result(i) == (p[i], r[i], ap[i, 0], ap[i, 5], ap[i].mean())
    assert ap[2].sum() == 0 and ap[0, 0] > ap[0, 9] > 0  # class 3: labels, no detections
    maps = m.maps
    assert maps.shape == (5,)
    assert maps[0] == ap[0].mean() and maps[2] == ap[1].mean() and maps[3] == 0
    assert maps[1] == maps[4] == b.map  # classes without labels get the mean (:753)
    cr = m.curves_results
    assert [c[2:] for c in cr] == [["Recall", "Precision"], ["Confidence", "F1"], ["Confidence", "Precision"],
                                  ["Confidence", "Recall"]]
    assert len(m.curves) == 4 and cr[1][1].shape == (3, 1000) and cr[0][1].shape == (2, 1000)
    # results_dict and its fitness stay as they were
    rd = m.results_dict
    assert list(rd) == m.keys + ["fitness"] and rd["fitness"] == 0.1 * b.map50 + 0.9 * b.map
    assert rd["metrics/mAP75(B)"] == b.map75


def test_pred_to_json_rows():
    from ydbl.engine.validator import pred_to_json

    predn = torch.tensor([[10.12345, 20.5, 110.98765, 220.25, 0.87654321, 2.0],
                          [0.0, 0.0, 1.0 / 3.0, 2.0 / 3.0, 0.123456789, 0.0]])
    rows = pred_to_json(predn, "/data/images/000000123.jpg")
    assert [set(r) for r in rows] == [{"image_id", "category_id", "bbox", "score"}] * 2
    assert rows[0]["image_id"] == 123 and isinstance(rows[0]["image_id"], int)
    assert [r["category_id"] for r in rows] == [3, 1]  # class + 1 (val.py:77)
    p = predn.tolist()
    w, h = predn[0, 2] - predn[0, 0], predn[0, 3] - predn[0, 1]
    cx, cy = (predn[0, 0] + predn[0, 2]) / 2, (predn[0, 1] + predn[0, 3]) / 2
    want = [round(v.item(), 3) for v in (cx - w / 2, cy - h / 2, w, h)]  # fp32 xyxy2xywh, then top-left
    assert rows[0]["bbox"] == want and rows[0]["score"] == round(p[0][4], 5)
    assert rows[1]["bbox"] == [0.0, 0.0, 0.333, 0.667] and rows[1]["score"] == 0.12346
    assert pred_to_json(predn, "im003.png")[0]["image_id"] == "im003"
    assert pred_to_json(predn[:0], "7.jpg") == []
    assert pred_to_json(predn, "7.jpg", class_map=[1, 2, 90])[0]["category_id"] == 90
    json.dumps(rows)  # plain Python numbers


@pytest.mark.parametrize("save_conf", [False, True])
def test_save_one_txt(tmp_path, save_conf):
    from ydbl.engine.validator import save_one_txt

    predn = torch.tensor([[10.0, 20.0, 110.0, 220.0, 0.875, 2.0], [0.0, 0.0, 50.0, 40.0, 0.5, 0.0]])
    f = tmp_path / "labels" / "im0.txt"
    save_one_txt(predn, save_conf, (400, 200), {0: "a", 1: "b", 2: "c"}, f)
    rows = [ln.split() for ln in f.read_text().splitlines()]
    assert [r[0] for r in rows] == ["2", "0"]
    assert [float(v) for v in rows[0][1:5]] == [0.3, 0.3, 0.5, 0.5]  # xc / 200, yc / 400, w / 200, h / 400
    assert [float(v) for v in rows[1][1:5]] == [0.125, 0.05, 0.25, 0.1]
    assert [len(r) for r in rows] == [6 if save_conf else 5] * 2
    if save_conf:
        assert [float(r[5]) for r in rows] == [0.875, 0.5]
    save_one_txt(predn[:0], save_conf, (400, 200), {}, tmp_path / "labels" / "none.txt")
    assert not (tmp_path / "labels" / "none.txt").exists()  # no detections: no file, as Results.save_txt


def test_confusion_matrix_host_side(caplog):
    from ydbl.utils.metrics import ConfusionMatrix

    cm = ConfusionMatrix(3, conf=0.001)
    assert cm.conf == 0.25 and cm.iou_thres == 0.45 and ConfusionMatrix(3, conf=0.4).conf == 0.4
    assert cm.matrix.shape == (4, 4) and cm.matrix.dtype == np.float64 and not cm.matrix.any()
    assert not hasattr(cm, "plot")
    given = np.array([[5, 1, 0, 2], [0, 7, 1, 0], [2, 0, 3, 4], [1, 1, 1, 0]], dtype=np.float64)
    cm.matrix = given
    tp, fp = cm.tp_fp()
    assert tp.tolist() == [5, 7, 3] and fp.tolist() == [3, 1, 6]  # row sums minus the diagonal, background dropped
    with caplog.at_level(logging.INFO, logger="ydbl"):
        lines = cm.print()
    assert lines == ["5.0 1.0 0.0 2.0", "0.0 7.0 1.0 0.0", "2.0 0.0 3.0 4.0", "1.0 1.0 1.0 0.0"]
    assert [r.getMessage() for r in caplog.records] == lines
    with pytest.raises(ValueError):
        cm.matrix = np.zeros((3, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        cm.process_batch(torch.zeros(2, 6), torch.zeros(1, 4), torch.zeros(1))
    cm.process_batch(None, torch.zeros(0, 4), torch.zeros(0))  # neither detections nor labels: nothing to do
    assert np.array_equal(cm.matrix, given)
