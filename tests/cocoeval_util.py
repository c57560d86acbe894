"""A plain numpy restatement of the COCO detection protocol for boxes without crowd labels — per-image evaluate,
accumulate, summarize, loop by loop — and a seeded scene generator for the tests of ydbl_coco_match and
val(coco_eval=True).  It shares no code with the product (ydbl.utils.metrics / csrc/cocoeval.hip).

Boxes are the fp32 xyxy rows the validator holds; each coordinate is converted to fp64 before anything else."""

import functools

import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 32**2], [32**2, 96**2], [96**2, 1e10]]
STAT_NAMES = ["mAP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]


def category(c, nc):
    """The category of a class value: truncation inside (-1, nc), -1 (no category) outside."""
    c = float(c)
    return int(c) if -1.0 < c < nc else -1


def xywh64(row):
    x1, y1, x2, y2 = (np.float64(v) for v in row[:4])
    return x1, y1, x2 - x1, y2 - y1


def iou64(d, g):
    dx, dy, dw, dh = d
    gx, gy, gw, gh = g
    iw = min(dx + dw, gx + gw) - max(dx, gx)
    ih = min(dy + dh, gy + gh) - max(dy, gy)
    if iw <= 0 or ih <= 0:
        return np.float64(0.0)
    i = iw * ih
    return i / (dw * dh + gw * gh - i)


def evaluate_pair(dets, scores, gts, iou_thrs=IOU_THRS, area_rng=AREA_RNG, cut=100):
    """One (image, category).  dets: xywh tuples in row order, scores their fp32 scores, gts: xywh tuples in label
    order.  Returns (order, dtm, dtig, gtig, taken): order = the row positions in score order cut to `cut`;
    dtm / dtig bool [A, T, D] over that order; gtig bool [A, G] in label order; taken int [A, T, D] = the label (in
    label order) each detection took, -1 for none; ties = the detections that meet two labels at one IoU >= 0.5."""
    order = sorted(range(len(dets)), key=lambda i: -float(scores[i]))[:cut]  # sorted() is stable
    A, T, D, G = len(area_rng), len(iou_thrs), len(order), len(gts)
    dtm, dtig = np.zeros((A, T, D), bool), np.zeros((A, T, D), bool)
    gtig, taken = np.zeros((A, G), bool), -np.ones((A, T, D), int)
    for a, (a0, a1) in enumerate(area_rng):
        for g in range(G):
            area = gts[g][2] * gts[g][3]
            gtig[a, g] = area < a0 or area > a1
        gorder = [g for g in range(G) if not gtig[a, g]] + [g for g in range(G) if gtig[a, g]]
        for t, thr in enumerate(iou_thrs):
            used = set()
            for di, row in enumerate(order):
                best, m = min(thr, 1 - 1e-10), -1
                for g in gorder:
                    if g in used:
                        continue
                    if m > -1 and not gtig[a, m] and gtig[a, g]:
                        break
                    v = iou64(dets[row], gts[g])
                    if v < best:
                        continue
                    best, m = v, g
                if m > -1:
                    used.add(m)
                    dtm[a, t, di], dtig[a, t, di], taken[a, t, di] = True, gtig[a, m], m
                else:
                    area = dets[row][2] * dets[row][3]
                    dtig[a, t, di] = area < a0 or area > a1
    ties = 0
    for row in order:
        v = [iou64(dets[row], g) for g in gts]
        ties += any(v[i] >= 0.5 and v[i] == v[j] for i in range(G) for j in range(i))
    return order, dtm, dtig, gtig, taken, ties


def evaluate_batch(det, cnt, boxes, cls, bidx, nc, single_cls=False, iou_thrs=IOU_THRS, area_rng=AREA_RNG, cut=100):
    """A batch as the kernel sees it.  det fp32 [n, max_det, 6], cnt [n], labels boxes [N, 4] / cls [N] / bidx [N] in
    any image order.  Returns (arrays, imgs):
    arrays — what ydbl_coco_match writes: rank int32 [n, max_det], matched / ignored int32 [n, max_det, A] (bit t),
    gt_ignore uint8 [N, A] with the labels grouped by image (stable), invalid int32 [n];
    imgs — per image {category: (scores [D] fp64, dtm [A, T, D], dtig [A, T, D], gtig [A, G], taken, IoU ties, rows
    the cut dropped)} for the categories that have labels or detections there."""
    det, cnt = np.asarray(det, np.float32), np.asarray(cnt).astype(int)
    boxes, cls = np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(cls, np.float32).reshape(-1)
    bidx = np.asarray(bidx).astype(int).reshape(-1)
    n, max_det = det.shape[:2]
    A, T = len(area_rng), len(iou_thrs)
    grouped = np.argsort(bidx, kind="stable")
    place = {int(orig): pos for pos, orig in enumerate(grouped)}
    rank = -np.ones((n, max_det), np.int32)
    matched, ignored = np.zeros((n, max_det, A), np.int32), np.zeros((n, max_det, A), np.int32)
    gt_ignore, invalid = np.zeros((len(cls), A), np.uint8), np.zeros(n, np.int32)
    for li in range(len(cls)):
        _, _, w, h = xywh64(boxes[li])
        for a, (a0, a1) in enumerate(area_rng):
            gt_ignore[place[li], a] = w * h < a0 or w * h > a1
    imgs = []
    for b in range(n):
        nd = min(max(int(cnt[b]), 0), max_det)
        rows_of, labels_of = {}, {}
        for d in range(nd):
            k = 0 if single_cls else category(det[b, d, 5], nc)
            if k < 0:
                invalid[b] += 1
            else:
                rows_of.setdefault(k, []).append(d)
        for li in np.nonzero(bidx == b)[0]:
            k = 0 if single_cls else category(cls[li], nc)
            if k >= 0:
                labels_of.setdefault(k, []).append(int(li))
        per = {}
        for k in sorted(set(rows_of) | set(labels_of)):
            rows, labs = rows_of.get(k, []), labels_of.get(k, [])
            order, dtm, dtig, gtig, taken, ties = evaluate_pair([xywh64(det[b, d]) for d in rows],
                                                          [det[b, d, 4] for d in rows],
                                                          [xywh64(boxes[li]) for li in labs], iou_thrs, area_rng, cut)
            for pos, o in enumerate(order):
                rank[b, rows[o]] = pos
                for a in range(A):
                    for t in range(T):
                        matched[b, rows[o], a] |= int(dtm[a, t, pos]) << t
                        ignored[b, rows[o], a] |= int(dtig[a, t, pos]) << t
            per[k] = (np.array([np.float64(det[b, rows[o], 4]) for o in order]), dtm, dtig, gtig, taken, ties,
                      len(rows) - len(order))
        imgs.append(per)
    return {"rank": rank, "matched": matched, "ignored": ignored, "gt_ignore": gt_ignore, "invalid": invalid}, imgs


def accumulate(imgs, nc, iou_thrs=IOU_THRS, rec_thrs=REC_THRS, max_dets=MAX_DETS, n_area=len(AREA_RNG)):
    """imgs: evaluate_batch's per-image dicts of every batch, in image order."""
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), nc, n_area, len(max_dets)
    precision, recall, scores = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), -np.ones((T, R, K, A, M))
    for k in range(K):
        E = [im[k] for im in imgs if k in im]
        if not E:
            continue
        for a in range(A):
            for m, md in enumerate(max_dets):
                sc = np.concatenate([e[0][:md] for e in E])
                inds = np.argsort(-sc, kind="mergesort")
                sc = sc[inds]
                dtm = np.concatenate([e[1][a][:, :md] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e[2][a][:, :md] for e in E], axis=1)[:, inds]
                npig = int(sum(np.count_nonzero(~e[3][a]) for e in E))
                if npig == 0:
                    continue
                for t in range(T):
                    tp = np.cumsum(np.logical_and(dtm[t], np.logical_not(dtig[t]))).astype(float)
                    fp = np.cumsum(np.logical_and(np.logical_not(dtm[t]), np.logical_not(dtig[t]))).astype(float)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q, ss = np.zeros(R), np.zeros(R)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thrs, side="left")):
                        if pi < nd:
                            q[ri], ss[ri] = pr[pi], sc[pi]
                    precision[t, :, k, a, m], scores[t, :, k, a, m] = q, ss
    return {"precision": precision, "recall": recall, "scores": scores}


def summarize(ev, iou_thrs=IOU_THRS):
    def stat(ap, thr=None, a=0, m=2):
        s = ev["precision"] if ap else ev["recall"]
        if thr is not None:
            s = s[np.where(np.isclose(iou_thrs, thr))[0]]
        s = s[..., a, m]
        return np.mean(s[s > -1]) if len(s[s > -1]) else -1.0

    return np.array([stat(1), stat(1, 0.5), stat(1, 0.75), stat(1, a=1), stat(1, a=2), stat(1, a=3),
                     stat(0, m=0), stat(0, m=1), stat(0, m=2), stat(0, a=1), stat(0, a=2), stat(0, a=3)], np.float64)


def run(batches, nc, single_cls=False):
    """(per-batch kernel arrays, eval dict, stats [12]) of a list of (det, cnt, boxes, cls, bidx) batches."""
    arrays, imgs = [], []
    for det, cnt, boxes, cls, bidx in batches:
        a, i = evaluate_batch(det, cnt, boxes, cls, bidx, nc, single_cls)
        arrays.append(a)
        imgs.extend(i)
    ev = accumulate(imgs, nc)
    return arrays, imgs, ev, summarize(ev)


def product_record(det, arrays, cls, bidx, nc, single_cls=False):
    """The numpy record ydbl.utils.metrics.coco_accumulate reads, from kernel-format arrays (the restatement's or
    the kernel's own)."""
    det = np.asarray(det, np.float32)
    cls = np.asarray(cls, np.float32).reshape(-1)[np.argsort(np.asarray(bidx).astype(int).reshape(-1), kind="stable")]
    dcat = np.array([[0 if single_cls else category(c, nc) for c in row] for row in det[..., 5]]).reshape(det.shape[:2])
    gcat = np.array([0 if single_cls else category(c, nc) for c in cls], dtype=int)
    return {"score": det[..., 4], "cls": dcat, "rank": np.asarray(arrays["rank"]),
            "matched": np.asarray(arrays["matched"]), "ignored": np.asarray(arrays["ignored"]), "gt_cls": gcat,
            "gt_ignore": np.asarray(arrays["gt_ignore"]).astype(bool)}


def xyxy(x, y, w, h):
    return [x, y, x + w, y + h]


def scene(n, max_det, nc, seed, empty_imgs=(), no_label_imgs=(), many_dets=None, many_labels=None, size=640.0):
    """A seeded batch with everything the protocol branches on.  Returns det fp32 [n, max_det, 6], cnt int32 [n],
    boxes [N, 4], cls [N], bidx [N] with the labels interleaved across images.

    Per image: labels in all three size bands (sides 8-28, 36-90, 100-300); per label one to three detections
    jittered so the IoUs spread over 0.5-0.95 and below; a fifth of the detections with a flipped class; scores drawn
    from a grid of 40 values, so ties within a category occur; one label box duplicated in its class, with a
    detection shifted so that it meets both at IoU 2/3 exactly (integer coordinates), and a pair of labels a
    detection meets at 0.6 each; a false positive of each size band far from every label; a medium-sized
    detection on a small label; one row with a class index outside [0, nc); rows past the count filled with garbage.  many_dets = (image, k): more than 100 detections of class k there; many_labels =
    (image, k): more than 64 labels of class k there.  empty_imgs have no detections, no_label_imgs no labels."""
    rng = np.random.default_rng(seed)
    det = rng.uniform(-1e3, 1e3, (n, max_det, 6)).astype(np.float32)  # garbage everywhere first
    det[..., 5] = rng.integers(-3, nc + 3, (n, max_det))
    cnt = np.zeros(n, np.int32)
    grid = np.linspace(0.05, 0.95, 40).astype(np.float32)
    boxes, cls = [[] for _ in range(n)], [[] for _ in range(n)]
    for b in range(n):
        rows = []

        def add(box, score, c):
            if len(rows) < max_det and b not in empty_imgs:
                rows.append([*box, score, c])

        labels = []
        if b not in no_label_imgs:
            for lo, hi in ((8, 28), (36, 90), (100, 300)):
                for _ in range(int(rng.integers(2, 5))):
                    w, h = rng.uniform(lo, hi, 2)
                    x, y = rng.uniform(0, size - w), rng.uniform(0, size - h)
                    labels.append((xyxy(x, y, w, h), int(rng.integers(0, nc))))
            # two 40 x 40 labels 20 px apart and a detection midway: IoU 30/50 with both (integer coordinates) ...
            c = int(rng.integers(0, nc))
            x, y = float(rng.integers(0, 400)), float(rng.integers(0, 400))
            labels += [(xyxy(x, y, 40.0, 40.0), c), (xyxy(x + 20.0, y, 40.0, 40.0), c)]
            add(xyxy(x + 10.0, y, 40.0, 40.0), grid[31], c)
            # ... and a duplicated 50 x 20 label with a detection 10 px aside: IoU 800/1200 = 2/3 with both, off every
            # threshold; the two detections tie in score
            x, y = float(rng.integers(0, 400)), float(rng.integers(400, 560))
            labels += [(xyxy(x, y, 50.0, 20.0), c), (xyxy(x, y, 50.0, 20.0), c)]
            add(xyxy(x + 10.0, y, 50.0, 20.0), grid[31], c)
            if many_labels and many_labels[0] == b:
                for j in range(70):
                    labels.append((xyxy(8.0 * j, 600.0, 7.0, 30.0), many_labels[1]))
        if b not in empty_imgs:
            for box, c in labels:
                x1, y1, x2, y2 = box
                w, h = x2 - x1, y2 - y1
                for _ in range(int(rng.integers(1, 4))):
                    j = rng.choice([0.0, 0.02, 0.05, 0.1, 0.2, 0.35])
                    dx, dy, sw, sh = rng.uniform(-j, j, 4)
                    cc = int(rng.integers(0, nc)) if rng.random() < 0.2 else c
                    add(xyxy(x1 + dx * w, y1 + dy * h, w * (1 + sw), h * (1 + sh)), rng.choice(grid), cc)
            for lo, hi in ((8, 28), (36, 90), (100, 300)):  # nothing to match: ignored outside their own band
                w, h = rng.uniform(lo, hi, 2)
                add(xyxy(size + rng.uniform(0, 200), size + rng.uniform(0, 200), w, h), rng.choice(grid),
                    int(rng.integers(0, nc)))
            # a medium-sized detection on a small label (IoU >= 0.5): matched to a label ignored in "medium"
            small = [bx for bx, _ in labels if (bx[2] - bx[0]) * (bx[3] - bx[1]) < 32**2]
            if small:
                x1, y1, x2, y2 = small[0]
                s = max(33.0 / min(x2 - x1, y2 - y1), 1.0)
                if s * s <= 1.9:
                    add(xyxy(x1, y1, (x2 - x1) * s, (y2 - y1) * s), grid[35],
                        [c for bx, c in labels if bx is small[0]][0])
            add(xyxy(10.0, 10.0, 50.0, 50.0), grid[20], nc + 1)  # a class of no category
            if many_dets and many_dets[0] == b:
                for j in range(130):
                    add(xyxy(5.0 * j, 5.0 * (j % 7), 30.0 + j % 5, 40.0), grid[j % 40], many_dets[1])
        rng.shuffle(rows)  # the NMS order is not assumed
        cnt[b] = len(rows)
        if rows:
            det[b, : len(rows)] = np.array(rows, np.float32)
        boxes[b] = [bx for bx, _ in labels]
        cls[b] = [c for _, c in labels]
    # interleave the labels across images, keeping each image's own order
    out_b, out_c, out_i = [], [], []
    j = 0
    while any(j < len(boxes[b]) for b in range(n)):
        for b in range(n):
            if j < len(boxes[b]):
                out_b.append(boxes[b][j])
                out_c.append(cls[b][j])
                out_i.append(b)
        j += 1
    return (det, cnt, np.array(out_b, np.float32).reshape(-1, 4), np.array(out_c, np.float32),
            np.array(out_i, np.int64))


# (n, max_det, nc, single_cls, scene keywords of each batch): the cases of tests/test_gpu_cocoeval.py.  The
# 2 x 64 x 80 case is two batches: an image without detections beside one without labels matches nothing, so a full
# batch goes first and the stats are taken over both.
SCENES = {
    "3x300x3": (3, 300, 3, False, [{"many_dets": (1, 2)}]),
    "2x64x80": (2, 64, 80, False, [{}, {"empty_imgs": (0,), "no_label_imgs": (1,)}]),
    "1x1000x2": (1, 1000, 2, False, [{"many_dets": (0, 1), "many_labels": (0, 1)}]),
    "4x300x3_single": (4, 300, 3, True, [{"many_dets": (2, 1)}]),
}


def make(name, seed=0):
    """(batches, nc, single_cls): each batch a (det, cnt, boxes, cls, bidx) of scene()."""
    n, max_det, nc, single, kws = SCENES[name]
    return [scene(n, max_det, nc, seed + 17 * n + max_det + 1000 * i, **kw) for i, kw in enumerate(kws)], nc, single


@functools.lru_cache(maxsize=None)
def reference(name):
    """(batches, nc, single_cls, arrays, imgs, ev, stats) of a named scene, computed once per process; read-only."""
    batches, nc, single = make(name)
    return (batches, nc, single, *run(batches, nc, single))


def census(imgs):
    """What a scene exercises, from evaluate_batch's per-image dicts: counts for the non-triviality check."""
    out = {"areas_with_labels": set(), "matched": 0, "unmatched": 0, "ig_matched": 0, "ig_unmatched": 0,
           "score_ties": 0, "iou_ties": 0, "cut": 0}
    for per in imgs:
        for k, (sc, dtm, dtig, gtig, taken, ties, dropped) in per.items():
            for a in range(gtig.shape[0]):
                if (~gtig[a]).any():
                    out["areas_with_labels"].add(a)
            out["matched"] += int((dtm & ~dtig).sum())
            out["unmatched"] += int((~dtm & ~dtig).sum())
            out["ig_matched"] += int((dtm & dtig).sum())
            out["ig_unmatched"] += int((~dtm & dtig).sum())
            out["score_ties"] += int(len(sc) - len(np.unique(sc)))
            out["iou_ties"] += int(ties)
            out["cut"] += int(dropped)
    return out
