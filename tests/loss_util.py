"""A torch-CPU restatement of the reference's detection loss, written from the cited lines, usable in fp32 and fp64:
v8DetectionLoss.__call__ (U/utils/loss.py:206-260) with bbox_decode (:197-204), BboxLoss (:99-113), DFLoss (:73-88),
bbox_iou(CIoU=True) (U/utils/metrics.py:74-134), TaskAlignedAssigner (U/utils/tal.py:40-295), make_anchors
(:333-345), dist2bbox (:348-357) and bbox2dist (:360-363).

``reference_loss`` returns the three losses, the per-image table, fg, target_gt_idx, the per-anchor target score and
two diagnostics: per label the relative gap between its 10th and 11th positive metric, and the number of anchors
selected by more than one label.  ``synthetic_case`` builds the inputs of tests/test_gpu_loss.py.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

TOPK, ALPHA, BETA, EPS = 10, 0.5, 6.0, 1e-9
REG_MAX = 16
GAINS = (7.5, 0.5, 1.5)  # U/cfg/default.yaml:99-101


def bbox_ciou(box1, box2, eps=1e-7):
    """bbox_iou(box1, box2, xywh=False, CIoU=True), U/utils/metrics.py:102-130."""
    b1_x1, b1_y1, b1_x2, b1_y2 = box1.chunk(4, -1)
    b2_x1, b2_y1, b2_x2, b2_y2 = box2.chunk(4, -1)
    w1, h1 = b1_x2 - b1_x1, b1_y2 - b1_y1 + eps
    w2, h2 = b2_x2 - b2_x1, b2_y2 - b2_y1 + eps
    inter = (b1_x2.minimum(b2_x2) - b1_x1.maximum(b2_x1)).clamp_(0) * (
        b1_y2.minimum(b2_y2) - b1_y1.maximum(b2_y1)).clamp_(0)
    union = w1 * h1 + w2 * h2 - inter + eps
    iou = inter / union
    cw = b1_x2.maximum(b2_x2) - b1_x1.minimum(b2_x1)
    ch = b1_y2.maximum(b2_y2) - b1_y1.minimum(b2_y1)
    c2 = cw.pow(2) + ch.pow(2) + eps
    rho2 = ((b2_x1 + b2_x2 - b1_x1 - b1_x2).pow(2) + (b2_y1 + b2_y2 - b1_y1 - b1_y2).pow(2)) / 4
    v = (4 / math.pi**2) * ((w2 / h2).atan() - (w1 / h1).atan()).pow(2)
    alpha = v / (v - iou + (1 + eps))
    return iou - (rho2 / c2 + v * alpha)


def make_anchors(shapes, strides, dtype, offset=0.5):
    """tal.py:333-345 for level shapes [(h, w), ...]."""
    pts, st = [], []
    for (h, w), s in zip(shapes, strides):
        sx = torch.arange(w, dtype=dtype) + offset
        sy = torch.arange(h, dtype=dtype) + offset
        sy, sx = torch.meshgrid(sy, sx, indexing="ij")
        pts.append(torch.stack((sx, sy), -1).view(-1, 2))
        st.append(torch.full((h * w, 1), s, dtype=dtype))
    return torch.cat(pts), torch.cat(st)


def assign(pd_scores, pd_bboxes, anc_points, gt_labels, gt_bboxes, mask_gt, topk=TOPK):
    """TaskAlignedAssigner._forward (tal.py:82-118).  Returns target_bboxes, target_scores, fg_mask, target_gt_idx
    and the diagnostics (align_metric before masking, the pre-resolution pick count per anchor)."""
    bs, n_max = gt_bboxes.shape[:2]
    na = pd_bboxes.shape[-2]
    # select_candidates_in_gts (:257-262)
    lt, rb = gt_bboxes.view(-1, 1, 4).chunk(2, 2)
    deltas = torch.cat((anc_points[None] - lt, rb - anc_points[None]), dim=2).view(bs, n_max, na, -1)
    mask_in_gts = deltas.amin(3).gt_(1e-9)
    # get_box_metrics (:132-151)
    m = (mask_in_gts * mask_gt).bool()
    overlaps = torch.zeros([bs, n_max, na], dtype=pd_bboxes.dtype)
    bbox_scores = torch.zeros([bs, n_max, na], dtype=pd_scores.dtype)
    ind0 = torch.arange(bs).view(-1, 1).expand(-1, n_max)
    ind1 = gt_labels.squeeze(-1).long()
    bbox_scores[m] = pd_scores[ind0, :, ind1][m]
    pd_b = pd_bboxes.unsqueeze(1).expand(-1, n_max, -1, -1)[m]
    gt_b = gt_bboxes.unsqueeze(2).expand(-1, -1, na, -1)[m]
    overlaps[m] = bbox_ciou(gt_b, pd_b).squeeze(-1).clamp_(0)
    align_metric = bbox_scores.pow(ALPHA) * overlaps.pow(BETA)
    # select_topk_candidates (:157-190)
    k = min(topk, na)
    _, topk_idxs = torch.topk(align_metric, k, dim=-1, largest=True)
    topk_idxs.masked_fill_(~mask_gt.expand(-1, -1, k).bool(), 0)
    count = torch.zeros(align_metric.shape, dtype=torch.int8)
    ones = torch.ones_like(topk_idxs[:, :, :1], dtype=torch.int8)
    for j in range(k):
        count.scatter_add_(-1, topk_idxs[:, :, j:j + 1], ones)
    count.masked_fill_(count > 1, 0)
    mask_pos = count.to(align_metric.dtype) * mask_in_gts * mask_gt
    picks = mask_pos.sum(-2).clone()
    # select_highest_overlaps (:265-295)
    fg_mask = mask_pos.sum(-2)
    if fg_mask.max() > 1:
        multi = (fg_mask.unsqueeze(1) > 1).expand(-1, n_max, -1)
        max_idx = overlaps.argmax(1)
        is_max = torch.zeros(mask_pos.shape, dtype=mask_pos.dtype)
        is_max.scatter_(1, max_idx.unsqueeze(1), 1)
        mask_pos = torch.where(multi, is_max, mask_pos).to(align_metric.dtype)
        fg_mask = mask_pos.sum(-2)
    target_gt_idx = mask_pos.argmax(-2)
    # get_targets (:192-238)
    nc = pd_scores.shape[-1]
    flat_idx = target_gt_idx + torch.arange(bs)[..., None] * n_max
    target_labels = gt_labels.long().flatten()[flat_idx].clamp_(0)
    target_bboxes = gt_bboxes.view(-1, 4)[flat_idx]
    target_scores = torch.zeros((bs, na, nc), dtype=torch.int64)
    target_scores.scatter_(2, target_labels.unsqueeze(-1), 1)
    target_scores = torch.where(fg_mask[:, :, None].repeat(1, 1, nc) > 0, target_scores, 0)
    # normalize (:111-116)
    raw_metric = align_metric.clone()
    align_metric = align_metric * mask_pos
    pos_align = align_metric.amax(dim=-1, keepdim=True)
    pos_ov = (overlaps * mask_pos).amax(dim=-1, keepdim=True)
    norm = (align_metric * pos_ov / (pos_align + EPS)).amax(-2).unsqueeze(-1)
    target_scores = target_scores * norm
    return target_bboxes, target_scores, fg_mask.bool(), target_gt_idx, raw_metric, picks


def reference_loss(box_logits, cls_logits, shapes, strides, gt, gains=GAINS, dtype=torch.float32, topk=TOPK):
    """box_logits [B, A, 64], cls_logits [B, A, nc] (anchors in level order, row-major), shapes [(h, w), ...],
    gt [B, M, 5] rows cls, x1, y1, x2, y2 in pixels, zero-padded.  Everything is computed in ``dtype``."""
    pred_distri, pred_scores = box_logits.to(dtype), cls_logits.to(dtype)
    gt = gt.to(dtype)
    B, A, nc = pred_scores.shape
    anchor_points, stride_tensor = make_anchors(shapes, strides, dtype)
    gt_labels, gt_bboxes = gt.split((1, 4), 2)
    mask_gt = gt_bboxes.sum(2, keepdim=True).gt_(0.0)
    proj = torch.arange(REG_MAX, dtype=dtype)
    dist = pred_distri.view(B, A, 4, REG_MAX).softmax(3).matmul(proj)  # bbox_decode (loss.py:197-204)
    lt, rb = dist.chunk(2, -1)
    pred_bboxes = torch.cat((anchor_points - lt, anchor_points + rb), -1)  # dist2bbox(xywh=False)
    out = {"loss": torch.zeros(3, dtype=dtype), "per_image": torch.zeros(B, 3, dtype=dtype)}
    if gt.shape[1] == 0:  # tal.py:64-71
        target_scores = torch.zeros_like(pred_scores)
        fg = torch.zeros(B, A, dtype=torch.bool)
        tgi = torch.zeros(B, A, dtype=torch.long)
        target_bboxes = torch.zeros_like(pred_bboxes)
        raw_metric, picks = torch.zeros(B, 0, A, dtype=dtype), torch.zeros(B, A, dtype=dtype)
    else:
        target_bboxes, target_scores, fg, tgi, raw_metric, picks = assign(
            pred_scores.sigmoid(), pred_bboxes * stride_tensor, anchor_points * stride_tensor, gt_labels, gt_bboxes,
            mask_gt, topk)
    tss = max(target_scores.sum(), 1)
    bce = F.binary_cross_entropy_with_logits(pred_scores, target_scores.to(dtype), reduction="none")
    box_img = torch.zeros(B, dtype=dtype)
    dfl_img = torch.zeros(B, dtype=dtype)
    if fg.sum():
        target_bboxes = target_bboxes / stride_tensor
        weight = target_scores.sum(-1)
        iou = bbox_ciou(pred_bboxes, target_bboxes).squeeze(-1)  # BboxLoss (:99-113); masked per image below
        box_terms = (1.0 - iou) * weight
        x1y1, x2y2 = target_bboxes.chunk(2, -1)
        ltrb = torch.cat((anchor_points - x1y1, x2y2 - anchor_points), -1).clamp_(0, REG_MAX - 1 - 0.01)  # bbox2dist
        t = ltrb.clamp(0, REG_MAX - 1 - 0.01)  # DFLoss (:73-88)
        tl = t.long()
        tr = tl + 1
        wl = tr - t
        wr = 1 - wl
        pd = pred_distri.view(B * A * 4, REG_MAX)
        ce_l = F.cross_entropy(pd, tl.view(-1), reduction="none").view(tl.shape)
        ce_r = F.cross_entropy(pd, tr.view(-1), reduction="none").view(tl.shape)
        dfl_terms = (ce_l * wl + ce_r * wr).mean(-1) * weight
        for b in range(B):
            box_img[b] = box_terms[b][fg[b]].sum()
            dfl_img[b] = dfl_terms[b][fg[b]].sum()
    g = torch.tensor(gains, dtype=dtype)
    per = torch.stack((box_img, bce.sum((1, 2)), dfl_img), 1) / tss * g
    # the totals as the reference sums them: over all fg anchors / all classes at once
    loss = torch.zeros(3, dtype=dtype)
    loss[1] = bce.sum() / tss
    if fg.sum():
        loss[0] = box_terms[fg].sum() / tss
        loss[2] = dfl_terms[fg].sum() / tss
    out["loss"], out["per_image"] = loss * g, per
    out["target_scores_sum"] = torch.as_tensor(tss, dtype=dtype)
    out["fg"], out["target_gt_idx"] = fg, tgi
    out["target_score"] = target_scores.sum(-1)  # the value on the label's class (one-hot rows)
    # diagnostics
    real = mask_gt.squeeze(-1).bool()
    gaps, short = [], 0
    for b in range(B):
        for m in range(gt.shape[1]):
            if not real[b, m]:
                continue
            pos = raw_metric[b, m][raw_metric[b, m] > 0].sort(descending=True).values
            if len(pos) > topk:
                gaps.append(float((pos[topk - 1] - pos[topk]) / pos[topk - 1]))
            # in-box anchors of this label
            d = torch.cat((anchor_points * stride_tensor - gt_bboxes[b, m, :2], gt_bboxes[b, m, 2:] -
                           anchor_points * stride_tensor), 1).amin(1)
            n_in = int((d > 1e-9).sum())
            short += int(n_in < topk)
            out.setdefault("in_box", []).append(n_in)
    out["gaps"], out["short_labels"] = gaps, short
    out["multi_selected"] = int((picks > 1).sum())
    return out


def level_shapes(h, w, strides=(8, 16, 32)):
    return [(h // s, w // s) for s in strides]


def random_labels(gen, counts, h, w, max_labels, nc, wr=(10, 60), hr=(10, 50)):
    """gt [B, max_labels, 5]: counts[b] boxes per image, wr / hr px wide / high, placed uniformly inside the input."""
    gt = torch.zeros(len(counts), max_labels, 5)
    for b, n in enumerate(counts):
        for m in range(n):
            bw = wr[0] + (wr[1] - wr[0]) * torch.rand((), generator=gen).item()
            bh = hr[0] + (hr[1] - hr[0]) * torch.rand((), generator=gen).item()
            bw, bh = min(bw, w - 1.0), min(bh, h - 1.0)
            x1 = (w - bw) * torch.rand((), generator=gen).item()
            y1 = (h - bh) * torch.rand((), generator=gen).item()
            c = int(torch.randint(0, nc, (), generator=gen))
            gt[b, m] = torch.tensor([c, x1, y1, x1 + bw, y1 + bh])
    return gt


def synthetic_case(seed, h=64, w=96, nc=3, counts=(6, 3, 0), max_labels=6, strides=(8, 16, 32)):
    """The recipe of tests/test_gpu_loss.py: box logits ~ 2 N(0,1), class logits ~ 1.5 N(0,1) - 2, per level one
    NHWC map [B, h_l, w_l, 64+nc] (what Detect.emit writes), and the labels."""
    gen = torch.Generator().manual_seed(seed)
    B = len(counts)
    shapes = level_shapes(h, w, strides)
    levels = []
    for lh, lw in shapes:
        box = 2.0 * torch.randn(B, lh, lw, 64, generator=gen)
        cls = 1.5 * torch.randn(B, lh, lw, nc, generator=gen) - 2.0
        levels.append(torch.cat((box, cls), -1))
    gt = random_labels(gen, counts, h, w, max_labels, nc)
    return levels, shapes, list(strides), gt


def flatten_levels(levels):
    """NHWC level maps -> (box_logits [B, A, 64], cls_logits [B, A, nc]) in anchor order."""
    B = levels[0].shape[0]
    flat = torch.cat([lv.reshape(B, -1, lv.shape[-1]) for lv in levels], 1)
    return flat[..., :64].contiguous(), flat[..., 64:].contiguous()


def rel_dist(a, b):
    """Largest |a - b| relative to the largest |b| (the scale of the quantity), as a float."""
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    if a.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
