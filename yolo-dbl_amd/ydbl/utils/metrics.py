"""Detection metrics for the mAP acceptance check (host numpy, as the reference computes them).

Restates U/utils/metrics.py:447-452 (smooth), :505-534 (compute_ap, 101-point COCO interpolation),
:537-623 (ap_per_class), :626-805 (Metric: per-class results, maps, curves) and :808-906 (DetMetrics, keys incl.
mAP75).  The per-image TP matrix (box_iou + match_predictions) runs on the device: ydbl_match_predictions, see
engine/validator.py; its host restatement is the checker in oracle/metrics.py.  ConfusionMatrix (:294-445) keeps
the reference's interface over a device accumulator that ydbl_confusion_matrix adds into.
coco_accumulate / coco_summarize restate COCOeval.accumulate / summarize (the protocol the reference reaches through
pycocotools, U/models/yolo/detect/val.py:297-337) over the per-image matching ydbl_coco_match does on the device.
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


# ---- COCO protocol (COCOeval's Params, accumulate and summarize for iouType "bbox") -------------------------------
COCO_IOU_THRS = np.linspace(0.5, 0.95, 10)
COCO_REC_THRS = np.linspace(0.0, 1.0, 101)
COCO_MAX_DETS = (1, 10, 100)
COCO_AREA_RNG = ((0.0, 1e10), (0.0, 32.0**2), (32.0**2, 96.0**2), (96.0**2, 1e10))
COCO_AREA_LBL = ("all", "small", "medium", "large")
COCO_STAT_NAMES = ("mAP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def coco_accumulate(batches, nc, iou_thrs=COCO_IOU_THRS, rec_thrs=COCO_REC_THRS, max_dets=COCO_MAX_DETS,
                    area_rng=COCO_AREA_RNG):
    """COCOeval.accumulate over the per-batch outputs of ydbl_coco_match (engine/validator.py coco_batch), host fp64.

    batches: dicts of numpy arrays in image order — ``score`` fp32 [B, max_det], ``cls`` int [B, max_det] (the
    category of each row), ``rank`` int32 [B, max_det] (-1: the row takes no part), ``matched`` / ``ignored`` int32
    [B, max_det, A] (bit t: at iou_thrs[t]), ``gt_cls`` int [N] (-1: a label of no category), ``gt_ignore`` bool
    [N, A].  Returns COCOeval's ``eval`` dict: precision [T, R, K, A, M], recall [T, K, A, M], scores like precision
    (-1 where a category has no non-ignored label in that area range), params and counts."""
    iou_thrs, rec_thrs = np.asarray(iou_thrs, np.float64), np.asarray(rec_thrs, np.float64)
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), int(nc), len(area_rng), len(max_dets)
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    img, cls, rank, score, dtm, dtig, gcls, gig = [], [], [], [], [], [], [], []
    i0 = 0
    for bt in batches:
        keep = np.asarray(bt["rank"]) >= 0
        bi, _ = np.nonzero(keep)
        img.append(bi + i0)
        i0 += keep.shape[0]
        cls.append(np.asarray(bt["cls"])[keep])
        rank.append(np.asarray(bt["rank"])[keep])
        score.append(np.asarray(bt["score"])[keep].astype(np.float64))
        dtm.append(np.asarray(bt["matched"])[keep])
        dtig.append(np.asarray(bt["ignored"])[keep])
        gcls.append(np.asarray(bt["gt_cls"]).reshape(-1))
        gig.append(np.asarray(bt["gt_ignore"]).reshape(-1, A).astype(bool))
    cat = lambda v, shape: np.concatenate(v) if v else np.zeros(shape)  # noqa: E731
    img, cls, rank, score = cat(img, 0), cat(cls, 0), cat(rank, 0), cat(score, 0)
    dtm, dtig, gcls, gig = cat(dtm, (0, A)), cat(dtig, (0, A)), cat(gcls, 0), cat(gig, (0, A)).astype(bool)
    order = np.lexsort((rank, img))  # image order, each image's category list in its score order
    img, cls, rank, score, dtm, dtig = img[order], cls[order], rank[order], score[order], dtm[order], dtig[order]
    bits = np.arange(T)[:, None]
    for k in range(K):
        sk = cls == k
        gk = gig[gcls == k]
        for m, md in enumerate(max_dets):
            sel = np.nonzero(sk & (rank < md))[0]
            sel = sel[np.argsort(-score[sel], kind="mergesort")]
            sc, nd = score[sel], len(sel)
            for a in range(A):
                npig = int(np.count_nonzero(~gk[:, a]))
                if npig == 0:
                    continue
                mt = ((dtm[sel, a][None, :] >> bits) & 1).astype(bool)
                ig = ((dtig[sel, a][None, :] >> bits) & 1).astype(bool)
                tps = np.cumsum(mt & ~ig, axis=1).astype(np.float64)
                fps = np.cumsum(~mt & ~ig, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tps[t], fps[t]
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                    idx = np.searchsorted(rc, rec_thrs, side="left")
                    ok = idx < nd
                    q, ss = np.zeros(R), np.zeros(R)
                    q[ok], ss[ok] = pr[idx[ok]], sc[idx[ok]]
                    precision[t, :, k, a, m], scores[t, :, k, a, m] = q, ss
    params = {"iouThrs": iou_thrs, "recThrs": rec_thrs, "maxDets": list(max_dets),
              "areaRng": [list(r) for r in area_rng], "areaRngLbl": list(COCO_AREA_LBL[:A]), "catIds": list(range(K)),
              "iouType": "bbox", "useCats": 1}
    return {"params": params, "counts": [T, R, K, A, M], "precision": precision, "recall": recall, "scores": scores}


def _coco_stat(ev, ap, iou_thr=None, area=0, max_det=-1):
    """COCOeval._summarize: the mean of the entries > -1 of one slice, -1 without any."""
    s = ev["precision"] if ap else ev["recall"]
    if iou_thr is not None:
        s = s[np.isclose(ev["params"]["iouThrs"], iou_thr)]
    s = s[..., area, max_det]
    return float(s[s > -1].mean()) if (s > -1).any() else -1.0


_COCO_ROWS = ((1, None, 0, 2), (1, 0.5, 0, 2), (1, 0.75, 0, 2), (1, None, 1, 2), (1, None, 2, 2), (1, None, 3, 2),
              (0, None, 0, 0), (0, None, 0, 1), (0, None, 0, 2), (0, None, 1, 2), (0, None, 2, 2), (0, None, 3, 2))


def coco_summarize(ev):
    """COCOeval.summarize for boxes: float64 [12] in the order of COCO_STAT_NAMES (needs the standard 4 area ranges
    and 3 maxDets)."""
    if ev["counts"][3] != 4 or ev["counts"][4] != 3:
        raise ValueError("coco_summarize needs the 4 standard area ranges and 3 maxDets")
    return np.array([_coco_stat(ev, *row) for row in _COCO_ROWS], dtype=np.float64)


def coco_summary_lines(ev):
    """The twelve lines COCOeval.summarize prints."""
    p = ev["params"]
    lines = []
    for ap, thr, a, m in _COCO_ROWS:
        iou = f"{p['iouThrs'][0]:0.2f}:{p['iouThrs'][-1]:0.2f}" if thr is None else f"{thr:0.2f}"
        lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if ap else "Average Recall", "(AP)" if ap else "(AR)", iou, p["areaRngLbl"][a],
            p["maxDets"][m], _coco_stat(ev, ap, thr, a, m)))
    return lines


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
    coco_stat_names = list(COCO_STAT_NAMES)
    loss_keys = ["val/box_loss", "val/cls_loss", "val/dfl_loss"]  # label_loss_items(prefix="val")

    def __init__(self, names=None):
        self.names = names or {}
        self.box = BoxMetric()
        self.speed = {}
        self.confusion_matrix = None
        # val(coco_eval=True): COCOeval's 12 stats (float64 [12]) and its eval dict; None otherwise
        self.coco_stats = self.coco_eval = None

    def process_coco(self, batches, nc):
        self.coco_eval = coco_accumulate(batches, nc)
        self.coco_stats = coco_summarize(self.coco_eval)

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
        d = dict(zip(self.keys + ["fitness"], [b.mp, b.mr, b.map50, b.map75, b.map, 0.1 * b.map50 + 0.9 * b.map]))
        val_loss = self.__dict__.get("val_loss")  # set by val(loss=True) only (U/engine/validator.py:205)
        if val_loss is not None:
            d.update(zip(self.loss_keys, val_loss))
        return d


def metric_fitness(m: BoxMetric) -> float:
    """Metric.fitness (U/utils/metrics.py:758-761) with this fork's weights, as DetMetrics.results_dict computes it:
    0.1 * mAP50 + 0.9 * mAP50-95."""
    return 0.1 * m.map50 + 0.9 * m.map


def mask_iou(mask1, mask2, eps=1e-7):
    """U/utils/metrics.py:137-153: mask1 [N, n], mask2 [M, n] flattened masks -> IoU [N, M].

    CPU tensors: the reference's expression (matmul, sums, division) on any values.  CUDA tensors: the masks are
    packed to bit planes with torch ops and ydbl_mask_iou counts popcount(AND) -- defined for 0 / 1 masks only
    (any nonzero element counts as 1), eps = 1e-7 and n <= 2^24, where it is bitwise the reference's fp32 result."""
    if mask1.is_cuda:
        from .ops import mask_iou_bits, pack_mask_bits

        if float(eps) != 1e-7:
            raise ValueError("mask_iou on the device is defined for eps = 1e-7 (ydbl_mask_iou)")
        if mask1.shape[1] != mask2.shape[1]:
            raise ValueError(f"mask_iou: masks of {mask1.shape[1]} and {mask2.shape[1]} elements")
        dev, (N, n), M = mask1.device, mask1.shape, mask2.shape[0]
        if N == 0 or M == 0:
            return torch.zeros((N, M), dtype=torch.float32, device=dev)
        g, p = pack_mask_bits(mask1), pack_mask_bits(mask2.to(dev))
        area = (mask1 != 0).sum(1).to(torch.int32)
        return mask_iou_bits(p, torch.zeros(1, dtype=torch.int64, device=dev),
                             torch.full((1,), M, dtype=torch.int32, device=dev), M, g,
                             torch.tensor([0, N], dtype=torch.int32, device=dev), area, (1, n))
    intersection = torch.matmul(mask1, mask2.T).clamp_(0)
    union = (mask1.sum(1)[:, None] + mask2.sum(1)[None]) - intersection
    return intersection / (union + eps)


class SegmentMetrics:
    """U/utils/metrics.py:909-1048 with this fork's mAP75 in both groups.  ``box`` and ``seg`` are BoxMetric;
    confusion_matrix, the COCO fields and val_loss are carried as DetMetrics carries them (all box-based, as in the
    reference)."""

    keys = [*DetMetrics.keys, "metrics/precision(M)", "metrics/recall(M)", "metrics/mAP50(M)", "metrics/mAP75(M)",
            "metrics/mAP50-95(M)"]
    curves = [*DetMetrics.curves, "Precision-Recall(M)", "F1-Confidence(M)", "Precision-Confidence(M)",
              "Recall-Confidence(M)"]
    coco_stat_names = list(COCO_STAT_NAMES)
    loss_keys = DetMetrics.loss_keys

    def __init__(self, names=None):
        self.names = names or {}
        self.box = BoxMetric()
        self.seg = BoxMetric()
        self.speed = {}
        self.task = "segment"
        self.confusion_matrix = None
        self.coco_stats = self.coco_eval = None

    process_coco = DetMetrics.process_coco

    def process(self, tp, tp_m, conf, pred_cls, target_cls):
        """:949-985: masks first, then boxes, each through ap_per_class."""
        self.seg.nc = len(self.names)
        self.seg.update(ap_per_class(tp_m, conf, pred_cls, target_cls, curves=True)[2:])
        self.box.nc = len(self.names)
        self.box.update(ap_per_class(tp, conf, pred_cls, target_cls, curves=True)[2:])

    def mean_results(self):
        return self.box.mean_results() + self.seg.mean_results()

    def class_result(self, i):
        return self.box.class_result(i) + self.seg.class_result(i)

    @property
    def maps(self):
        return self.box.maps + self.seg.maps

    @property
    def fitness(self):
        return metric_fitness(self.seg) + metric_fitness(self.box)

    @property
    def ap_class_index(self):
        return self.box.ap_class_index

    @property
    def curves_results(self):
        return self.box.curves_results + self.seg.curves_results

    @property
    def results_dict(self):
        d = dict(zip(self.keys + ["fitness"], self.mean_results() + [self.fitness]))
        val_loss = self.__dict__.get("val_loss")
        if val_loss is not None:
            d.update(zip(self.loss_keys, val_loss))
        return d


# The COCO keypoint evaluation's per-keypoint scales (nose, eyes, ears, shoulders, elbows, wrists, hips, knees, ankles),
# U/utils/metrics.py:15-18: the published COCO sigmas.
OKS_SIGMA = np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89,
                      0.89]) / 10.0


def kpt_iou(kpt1, kpt2, area, sigma, eps=1e-7):
    """U/utils/metrics.py:156-175 (OKS): kpt1 [N, K, 3] ground truth, kpt2 [M, K, >= 2] predictions, area [N], sigma
    [K] -> [N, M], in torch on the tensors' device and dtype.  (The validator's batch form is ydbl_kpt_oks.)"""
    d = (kpt1[:, None, :, 0] - kpt2[..., 0]).pow(2) + (kpt1[:, None, :, 1] - kpt2[..., 1]).pow(2)
    sigma = torch.as_tensor(np.asarray(sigma), device=kpt1.device).to(kpt1.dtype)
    kpt_mask = kpt1[..., 2] != 0
    e = d / ((2 * sigma).pow(2) * (area[:, None, None] + eps) * 2)
    return ((-e).exp() * kpt_mask[:, None]).sum(-1) / (kpt_mask.sum(-1)[:, None] + eps)


class PoseMetrics(SegmentMetrics):
    """U/utils/metrics.py:1051-1165 with this fork's mAP75 in both groups, as SegmentMetrics: ``box`` and ``pose`` are
    BoxMetric, fitness = pose + box."""

    keys = [*DetMetrics.keys, "metrics/precision(P)", "metrics/recall(P)", "metrics/mAP50(P)", "metrics/mAP75(P)",
            "metrics/mAP50-95(P)"]
    curves = [*DetMetrics.curves, "Precision-Recall(P)", "F1-Confidence(P)", "Precision-Confidence(P)",
              "Recall-Confidence(P)"]

    def __init__(self, names=None):
        super().__init__(names)
        self.pose = self.seg  # the second group under its own name (the shared methods read self.seg)
        self.task = "pose"

    def process(self, tp, tp_p, conf, pred_cls, target_cls):
        """:1096-1131: keypoints first, then boxes, each through ap_per_class."""
        super().process(tp, tp_p, conf, pred_cls, target_cls)


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
