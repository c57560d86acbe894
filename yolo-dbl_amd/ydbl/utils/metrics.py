"""Detection metrics for the mAP acceptance check (host numpy, as the reference computes them).

Restates U/utils/metrics.py:447-452 (smooth), :505-534 (compute_ap, 101-point COCO interpolation),
:537-623 (ap_per_class), :626-805 (Metric: per-class results, maps, curves) and :808-906 (DetMetrics, keys incl.
mAP75).  The per-image TP matrix (box_iou + match_predictions) runs on the device: ydbl_match_predictions, see
engine/validator.py; its host restatement is the checker in oracle/metrics.py.  ConfusionMatrix (:294-445) keeps
the reference's interface over a device accumulator that ydbl_confusion_matrix adds into.
"""

from __future__ import annotations

import logging

import numpy as np
import torch

LOGGER = logging.getLogger("ydbl")

IOUV = torch.linspace(0.5, 0.95, 10)  # U/models/yolo/detect/val.py:36 (iou vector for mAP@0.5:0.95)

_trapz = getattr(np, "trapezoid", None) or np.trapz


def smooth(y, f=0.05):
    """U/utils/metrics.py:447-452."""
    nf = round(len(y) * f * 2) // 2 + 1
    p = np.ones(nf // 2)
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def compute_ap(recall, precision):
    """U/utils/metrics.py:505-534 (101-point interpolation)."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    ap = _trapz(np.interp(x, mrec, mpre), x)
    return ap, mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, eps=1e-16, curves=False):
    """U/utils/metrics.py:537-623 without plotting. Returns (tp, fp, p, r, f1, ap, unique_classes); with
    curves=True the reference's remaining five follow: p_curve, r_curve, f1_curve [nc, 1000] over the confidence
    axis x [1000], and prec_values (precision over recall at IoU 0.5, one row per class that has predictions)."""
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes, nt = np.unique(target_cls, return_counts=True)
    nc = unique_classes.shape[0]
    x, prec_values = np.linspace(0, 1, 1000), []
    ap, p_curve, r_curve = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l = nt[ci]
        n_p = i.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + eps)
        r_curve[ci] = np.interp(-x, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p_curve[ci] = np.interp(-x, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j], mpre, mrec = compute_ap(recall[:, j], precision[:, j])
            if j == 0 and curves:
                prec_values.append(np.interp(x, mrec, mpre))
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    i = smooth(f1_curve.mean(0), 0.1).argmax()
    p, r, f1 = p_curve[:, i], r_curve[:, i], f1_curve[:, i]
    tp = (r * nt).round()
    fp = (tp / (p + eps) - tp).round()
    out = (tp, fp, p, r, f1, ap, unique_classes.astype(int))
    return out + (p_curve, r_curve, f1_curve, x, np.array(prec_values)) if curves else out


class BoxMetric:
    """U/utils/metrics.py:626-805 Metric: per-class P / R / F1 / AP, their means, and the curves."""

    def __init__(self):
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = [], [], [], [], []
        self.p_curve, self.r_curve, self.f1_curve, self.px, self.prec_values = [], [], [], [], []
        self.nc = 0

    def update(self, results):
        """(p, r, f1, all_ap, ap_class_index) or those plus (p_curve, r_curve, f1_curve, px, prec_values)."""
        self.p, self.r, self.f1, self.all_ap, self.ap_class_index = results[:5]
        if len(results) > 5:
            self.p_curve, self.r_curve, self.f1_curve, self.px, self.prec_values = results[5:]

    @property
    def ap50(self):
        return self.all_ap[:, 0] if len(self.all_ap) else []

    @property
    def ap75(self):
        return self.all_ap[:, 5] if len(self.all_ap) else []

    @property
    def ap(self):
        return self.all_ap.mean(1) if len(self.all_ap) else []

    @property
    def map50(self):
        return float(self.all_ap[:, 0].mean()) if len(self.all_ap) else 0.0

    @property
    def map75(self):
        return float(self.all_ap[:, 5].mean()) if len(self.all_ap) else 0.0

    @property
    def map(self):
        return float(self.all_ap.mean()) if len(self.all_ap) else 0.0

    @property
    def mp(self):
        return float(self.p.mean()) if len(self.p) else 0.0

    @property
    def mr(self):
        return float(self.r.mean()) if len(self.r) else 0.0

    def mean_results(self):
        """:742-744 of this fork: mp, mr, map50, map75, map."""
        return [self.mp, self.mr, self.map50, self.map75, self.map]

    def class_result(self, i):
        """:746-748: p[i], r[i], ap50[i], ap75[i], ap[i] of the i-th class that has labels (ap_class_index[i])."""
        return self.p[i], self.r[i], self.ap50[i], self.ap75[i], self.ap[i]

    @property
    def maps(self):
        """:750-756: mAP50-95 per class index; classes without labels get the mean."""
        maps = np.zeros(self.nc) + self.map
        for i, c in enumerate(self.ap_class_index):
            maps[c] = self.ap[i]
        return maps

    @property
    def curves_results(self):
        """:797-805."""
        return [[self.px, self.prec_values, "Recall", "Precision"], [self.px, self.f1_curve, "Confidence", "F1"],
                [self.px, self.p_curve, "Confidence", "Precision"], [self.px, self.r_curve, "Confidence", "Recall"]]


class DetMetrics:
    """U/utils/metrics.py:808-906 (keys include mAP75, :866-868).  confusion_matrix is set by the validator."""

    keys = ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP75(B)", "metrics/mAP50-95(B)"]
    curves = ["Precision-Recall(B)", "F1-Confidence(B)", "Precision-Confidence(B)", "Recall-Confidence(B)"]

    def __init__(self, names=None):
        self.names = names or {}
        self.box = BoxMetric()
        self.speed = {}
        self.confusion_matrix = None

    def process(self, tp, conf, pred_cls, target_cls):
        res = ap_per_class(tp, conf, pred_cls, target_cls, curves=True)
        self.box.nc = len(self.names)
        self.box.update(res[2:])

    def mean_results(self):
        return self.box.mean_results()

    def class_result(self, i):
        return self.box.class_result(i)

    @property
    def maps(self):
        return self.box.maps

    @property
    def ap_class_index(self):
        return self.box.ap_class_index

    @property
    def curves_results(self):
        return self.box.curves_results

    @property
    def results_dict(self):
        b = self.box
        return dict(zip(self.keys + ["fitness"], [b.mp, b.mr, b.map50, b.map75, b.map, 0.1 * b.map50 + 0.9 * b.map]))


class ConfusionMatrix:
    """U/utils/metrics.py:294-445 for detection, counted on the device by ydbl_confusion_matrix.

    Row = predicted class, column = true class, index nc = background.  ``matrix`` is a float64 numpy
    (nc+1, nc+1) array like the reference's; reading it copies the device accumulator back (and raises the
    reference's IndexError if a class outside [0, nc) was met).  Assigning to it replaces the counts.
    There is no plot(): plotting is out of scope."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        self.nc = nc
        self.conf = 0.25 if conf in {None, 0.001} else conf  # :311
        self.iou_thres = iou_thres
        self._base = np.zeros((nc + 1, nc + 1))
        self._acc = self._invalid = None  # device int64 [(nc+1)^2] / int32 [1], made on the first batch

    def buffers(self, device):
        """The device accumulator and invalid-class counter ydbl_confusion_matrix adds into."""
        if self._acc is None:
            self._acc = torch.zeros((self.nc + 1) ** 2, dtype=torch.int64, device=device)
            self._invalid = torch.zeros(1, dtype=torch.int32, device=device)
        elif self._acc.device != torch.device(device):
            raise RuntimeError(f"ConfusionMatrix accumulates on {self._acc.device}; got a batch on {device}")
        return self._acc, self._invalid

    @property
    def matrix(self):
        if self._acc is None:
            return self._base
        if int(self._invalid.item()):
            raise IndexError(f"{int(self._invalid.item())} confusion-matrix counts had a class outside [0, {self.nc})")
        return self._base + self._acc.cpu().numpy().reshape(self.nc + 1, self.nc + 1)

    @matrix.setter
    def matrix(self, value):
        value = np.asarray(value, dtype=np.float64)
        if value.shape != (self.nc + 1, self.nc + 1):
            raise ValueError(f"matrix must be {(self.nc + 1, self.nc + 1)}, got {value.shape}")
        self._base, self._acc, self._invalid = value, None, None

    def process_batch(self, detections, gt_bboxes, gt_cls):
        """One image (:326-382): detections [N, 6] (x1, y1, x2, y2, conf, cls) GPU tensor or None, gt_bboxes
        [M, 4] xyxy, gt_cls [M]."""
        from ..engine.validator import confusion_batch

        gt_cls = torch.as_tensor(gt_cls).reshape(-1)
        if detections is None:
            if gt_cls.shape[0] == 0:
                return
            dev = gt_cls.device if gt_cls.device.type == "cuda" else torch.device("cuda")
            detections = torch.zeros((0, 6), device=dev)
        if detections.device.type != "cuda":
            raise RuntimeError("process_batch runs on the GPU (ydbl_confusion_matrix); got a CPU tensor")
        n = detections.shape[0]
        det = torch.zeros((1, max(n, 1), 6), dtype=torch.float32, device=detections.device)
        det[0, :n] = detections[:, :6]
        count = torch.tensor([n], dtype=torch.int32, device=detections.device)
        confusion_batch(det, count, gt_bboxes, gt_cls, torch.zeros(gt_cls.shape[0], dtype=torch.long), self)

    def tp_fp(self):
        """:388-393: true and false positives per class (background dropped)."""
        m = self.matrix
        tp = m.diagonal()
        fp = m.sum(1) - tp
        return tp[:-1], fp[:-1]

    def print(self):
        """:441-444: one line per row; returns the lines it logged."""
        m = self.matrix
        lines = [" ".join(map(str, m[i])) for i in range(self.nc + 1)]
        for ln in lines:
            LOGGER.info(ln)
        return lines
