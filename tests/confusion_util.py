"""CPU checker for ydbl_confusion_matrix and random scenes for it (test infrastructure).

process_batch restates ConfusionMatrix.process_batch (U/utils/metrics.py:326-382) line by line in torch / numpy on
the CPU; confusion_reference sums it over the images of a batch the way DetectionValidator.update_metrics calls it
(U/models/yolo/detect/val.py:140-159).  The two threshold compares are torch's own (fp32 tensor against a Python
float), so their semantics are torch's and not ours.
"""

from __future__ import annotations

import numpy as np
import torch

from oracle.metrics import box_iou


def _bump(matrix, row, col, nc, skipped):
    """matrix[row, col] += 1, None standing for the background index nc.  A class outside [0, nc) raises like
    the reference's index would, or, with a `skipped` list, is left out and noted there."""
    row, col = (nc if v is None else int(v) if 0 <= int(v) < nc else -1 for v in (row, col))
    if row >= 0 and col >= 0:
        matrix[row, col] += 1
    elif skipped is None:
        raise IndexError(f"class outside [0, {nc})")
    else:
        skipped.append((row, col))


def process_batch(matrix, nc, conf, iou_thres, detections, gt_bboxes, gt_cls, skipped=None, kind=None):
    """One image into `matrix` (float64 numpy [nc+1, nc+1], row = predicted, column = true, nc = background).

    kind: the argsort kind.  None is the reference's call as it stands; its order on bit-equal IoUs is defined
    only for the small arrays numpy sorts by insertion (up to 16 rows), where it is the reversed stable order.
    "stable" asks for that order at any size: the larger label index takes a tied detection, the larger
    detection index a tied label — the rule ydbl_confusion_matrix documents.  Inputs that are not tie-free (a
    multi-label NMS keeps one box once per class, so real validator outputs are not) are checked with it."""
    if gt_cls.shape[0] == 0:  # :337-343 no labels: every kept detection is a false positive
        if detections is not None:
            detections = detections[detections[:, 4] > conf]
            for dc in detections[:, 5].int():
                _bump(matrix, dc, None, nc, skipped)
        return
    if detections is None:  # :344-348 no detections: every label is a background false negative
        for gc in gt_cls.int():
            _bump(matrix, None, gc, nc, skipped)
        return
    detections = detections[detections[:, 4] > conf]  # :350
    gt_classes = gt_cls.int()
    detection_classes = detections[:, 5].int()
    iou = box_iou(gt_bboxes, detections[:, :4])  # :357
    x = torch.where(iou > iou_thres)  # :360
    if x[0].shape[0]:
        matches = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()  # label, det, iou
        if x[0].shape[0] > 1:
            matches = matches[matches[:, 2].argsort(kind=kind)[::-1]]
            matches = matches[np.unique(matches[:, 1], return_index=True)[1]]  # the best label of each detection
            matches = matches[matches[:, 2].argsort(kind=kind)[::-1]]
            matches = matches[np.unique(matches[:, 0], return_index=True)[1]]  # the best detection of each label
    else:
        matches = np.zeros((0, 3))
    n = matches.shape[0] > 0
    m0, m1, _ = matches.transpose().astype(int)
    for i, gc in enumerate(gt_classes):  # :373-378
        j = m0 == i
        if n and sum(j) == 1:
            _bump(matrix, detection_classes[m1[j]], gc, nc, skipped)
        else:
            _bump(matrix, None, gc, nc, skipped)
    for i, dc in enumerate(detection_classes):  # :380-382
        if not any(m1 == i):
            _bump(matrix, dc, None, nc, skipped)


def confusion_reference(det, cnt, boxes, cls, bidx, nc, conf=0.25, iou_thres=0.45, single_cls=False, skipped=None,
                        kind=None):
    """The batch summed image by image as update_metrics does (val.py:140-159): an image without predictions
    counts its labels as missed (detections=None), single_cls zeroes the predicted classes first."""
    conf = 0.25 if conf in {None, 0.001} else conf  # :311
    matrix = np.zeros((nc + 1, nc + 1))
    for b in range(det.shape[0]):
        k = min(int(cnt[b]), det.shape[1])
        sel = bidx == b
        p = det[b, :k].clone().float()
        if single_cls:
            p[:, 5] = 0
        if k == 0:
            if sel.any():
                process_batch(matrix, nc, conf, iou_thres, None, boxes[sel].float(), cls[sel].float(), skipped, kind)
            continue
        process_batch(matrix, nc, conf, iou_thres, p, boxes[sel].float(), cls[sel].float(), skipped, kind)
    return matrix


def assert_tie_free(det, cnt, boxes, cls, bidx, conf=0.25, iou_thres=0.45):
    """A condition on the inputs: no two participating pairs that share a detection, or share a label, have
    bit-equal IoU, so the reference's unspecified sort order on ties cannot decide a cell."""
    for b in range(det.shape[0]):
        p = det[b, : int(cnt[b])]
        p = p[p[:, 4] > conf]
        sel = bidx == b
        if not len(p) or not sel.any():
            continue
        iou = box_iou(boxes[sel].float(), p[:, :4].float())
        part = iou > iou_thres
        for line, mask in list(zip(iou, part)) + list(zip(iou.t(), part.t())):
            v = line[mask]
            assert len(torch.unique(v)) == len(v), f"image {b}: bit-equal participating IoUs"


def assert_not_trivial(matrix, nc):
    """Every kind of cell is populated: diagonal, off-diagonal, background row (missed) and column (false positive)."""
    real = matrix[:nc, :nc]
    assert np.trace(real) > 0 and real.sum() - np.trace(real) > 0, "diagonal / off-diagonal empty"
    assert matrix[nc, :nc].sum() > 0 and matrix[:nc, nc].sum() > 0, "background row / column empty"
    assert matrix[nc, nc] == 0


def scene(n, max_det, nc, seed, empty_imgs=(), no_label_imgs=(), labels=(4, 40)):
    """Random detections jittered around random labels, like _scene of test_gpu_val.py, with random confidences so
    the 0.25 cut removes rows, a fifth of the classes flipped (off-diagonal cells), a few labels no detection is
    drawn from (missed) and a few detections far from every label (false positives).
    Returns det [n, max_det, 6], cnt int32 [n], boxes [N, 4], cls [N], bidx [N]."""
    g = torch.Generator().manual_seed(seed)
    det = torch.zeros(n, max_det, 6)
    cnt = torch.zeros(n, dtype=torch.int32)
    boxes, cls, bidx = [], [], []
    for b in range(n):
        nl = 0 if b in no_label_imgs else int(torch.randint(labels[0], labels[1], (1,), generator=g))
        xy = torch.rand(nl, 2, generator=g) * 500
        wh = torch.rand(nl, 2, generator=g) * 120 + 2
        lonely = torch.arange(nl) >= nl - max(nl // 5, 1)  # the last fifth: moved away, never a detection's source
        xy[lonely] += 2000
        gb = torch.cat([xy, xy + wh], 1)
        gc = torch.randint(0, nc, (nl,), generator=g).float()
        boxes.append(gb); cls.append(gc); bidx.append(torch.full((nl,), b))
        k = 0 if b in empty_imgs else int(torch.randint(max(max_det // 2, 1), max_det + 1, (1,), generator=g))
        if k:
            near = int((~lonely).sum())
            src = torch.randint(0, max(near, 1), (k,), generator=g)
            base = gb[src] if near else torch.rand(k, 4, generator=g) * 300
            jit = (torch.rand(k, 4, generator=g) - 0.5) * 40 * torch.rand(k, 1, generator=g)
            pb = base + jit
            far = torch.rand(k, generator=g) < 0.05
            pb[far] += 5000
            pb[:, 2:] = torch.maximum(pb[:, 2:], pb[:, :2] + 0.5)
            pc = gc[src] if near else torch.zeros(k)
            flip = torch.rand(k, generator=g) < 0.2
            pc = torch.where(flip, torch.randint(0, nc, (k,), generator=g).float(), pc)
            conf = torch.sort(torch.rand(k, generator=g), descending=True).values
            det[b, :k] = torch.cat([pb, conf[:, None], pc[:, None]], 1)
            det[b, k:] = 7.0  # garbage past the count (confidence 7, class 7) must be ignored
        cnt[b] = k
    return det, cnt, torch.cat(boxes), torch.cat(cls), torch.cat(bidx)


def pseudo_labels(det, cnt, size, cut=0.05, per_image=6):
    """Labels made from a batch's own detections above `cut`: up to six mutually dissimilar boxes of each image
    (IoU < 0.3 with those already taken), shifted by a fraction of a pixel to a few pixels, every third with
    another of three classes, plus one small corner box that is most likely missed."""
    boxes, cls, bidx = [], [], []
    for b in range(det.shape[0]):
        p = det[b, : int(cnt[b])]
        p = p[p[:, 4] > cut]
        chosen = []
        for j in range(len(p)):
            if len(chosen) == per_image:
                break
            if not chosen or box_iou(p[j: j + 1, :4], p[chosen, :4]).max() < 0.3:
                chosen.append(j)
        top = p[chosen]
        i = torch.arange(len(top))
        bb = (top[:, :4] + torch.tensor([0.37, -0.61, 0.83, 0.29]) * (1 + i[:, None])).clamp(0, size)
        keep = (bb[:, 2] - bb[:, 0] > 1) & (bb[:, 3] - bb[:, 1] > 1)
        cc = torch.where(i % 3 == 2, (top[:, 5] + 1) % 3, top[:, 5])
        boxes += [bb[keep], torch.tensor([[3.0, 3.0, 9.0, 9.0]]) + b]
        cls += [cc[keep], torch.tensor([float(b % 3)])]
        bidx += [torch.full((int(keep.sum()),), b), torch.tensor([b])]
    return torch.cat(boxes), torch.cat(cls), torch.cat(bidx)
