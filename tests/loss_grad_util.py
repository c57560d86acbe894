"""A torch restatement of the differentiable part of the reference's detection loss, for a GIVEN assignment, built so
that torch autograd reproduces the reference's gradient: v8DetectionLoss.__call__ (U/utils/loss.py:245-260) with
bbox_decode (:197-204), BboxLoss (:99-113), DFLoss (:73-88) and bbox_iou(xywh=False, CIoU=True)
(U/utils/metrics.py:102-130), whose ``alpha`` is computed under ``torch.no_grad()`` (:128-129).  The assigner's outputs
-- fg, target_gt_idx, the per-anchor target score and target_scores_sum -- are constants, as in the reference, where
the assigner runs under no_grad on detached inputs (U/utils/loss.py:233-243).

``loss_util.reference_loss`` cannot serve: it differentiates through alpha and through the assigner.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from loss_util import GAINS, REG_MAX, make_anchors


def bbox_ciou_const_alpha(box1, box2, eps=1e-7):
    """bbox_iou(box1, box2, xywh=False, CIoU=True), U/utils/metrics.py:102-130, alpha under no_grad (:128-129)."""
    b1_x1, b1_y1, b1_x2, b1_y2 = box1.chunk(4, -1)
    b2_x1, b2_y1, b2_x2, b2_y2 = box2.chunk(4, -1)
    w1, h1 = b1_x2 - b1_x1, b1_y2 - b1_y1 + eps
    w2, h2 = b2_x2 - b2_x1, b2_y2 - b2_y1 + eps
    inter = (b1_x2.minimum(b2_x2) - b1_x1.maximum(b2_x1)).clamp(0) * (
        b1_y2.minimum(b2_y2) - b1_y1.maximum(b2_y1)).clamp(0)
    union = w1 * h1 + w2 * h2 - inter + eps
    iou = inter / union
    cw = b1_x2.maximum(b2_x2) - b1_x1.minimum(b2_x1)
    ch = b1_y2.maximum(b2_y2) - b1_y1.minimum(b2_y1)
    c2 = cw.pow(2) + ch.pow(2) + eps
    rho2 = ((b2_x1 + b2_x2 - b1_x1 - b1_x2).pow(2) + (b2_y1 + b2_y2 - b1_y1 - b1_y2).pow(2)) / 4
    v = (4 / math.pi**2) * ((w2 / h2).atan() - (w1 / h1).atan()).pow(2)
    with torch.no_grad():
        alpha = v / (v - iou + (1 + eps))
    return iou - (rho2 / c2 + v * alpha)


def given_assignment_loss(box_logits, cls_logits, shapes, strides, gt, fg, target_gt_idx, target_score,
                          target_scores_sum, gains=GAINS, dtype=torch.float64):
    """box_logits [B, A, 64], cls_logits [B, A, nc] (may require grad), shapes [(h, w), ...], strides, gt [B, M, 5]
    rows cls, x1, y1, x2, y2 in pixels; the assignment: fg [B, A] bool, target_gt_idx [B, A], target_score [B, A] (the
    value on the label's class), target_scores_sum (scalar).  Returns (total, terms): total = loss.sum() * B as the
    reference returns it, terms = the three losses times their gains.  Everything is computed in ``dtype``."""
    pred_distri, pred_scores = box_logits.to(dtype), cls_logits.to(dtype)
    B, A, nc = pred_scores.shape
    dev = pred_scores.device  # (the CPU in the tests; scripts/loss_grad_timing.py runs it on the GPU)
    gt = gt.detach().to(dev, dtype)
    fg = fg.detach().to(dev).bool()
    tgi = target_gt_idx.detach().to(dev).long().clamp(0, max(gt.shape[1] - 1, 0))
    weight = torch.where(fg, target_score.detach().to(dev, dtype), torch.zeros((), dtype=dtype, device=dev))
    tss = torch.as_tensor(target_scores_sum).detach().to(dev, dtype).reshape(())
    anchor_points, stride_tensor = (t.to(dev) for t in make_anchors(shapes, strides, dtype))
    # the targets (tal.py:192-238), from the given assignment
    if gt.shape[1]:
        rows = gt[torch.arange(B, device=dev)[:, None], tgi]  # [B, A, 5]
    else:
        rows = torch.zeros(B, A, 5, dtype=dtype, device=dev)
    labels = rows[..., 0].long().clamp(0, nc - 1)
    target_scores = F.one_hot(labels, nc).to(dtype) * weight[..., None]
    target_bboxes = rows[..., 1:5] / stride_tensor
    # bbox_decode (loss.py:197-204)
    proj = torch.arange(REG_MAX, dtype=dtype, device=dev)
    dist = pred_distri.reshape(B, A, 4, REG_MAX).softmax(3).matmul(proj)
    lt, rb = dist.chunk(2, -1)
    pred_bboxes = torch.cat((anchor_points - lt, anchor_points + rb), -1)
    zero = pred_distri.sum() * 0  # (keeps the box logits in the graph when nothing is fg: their gradient is 0)
    cls_term = F.binary_cross_entropy_with_logits(pred_scores, target_scores, reduction="none").sum() / tss
    box_term, dfl_term = zero, zero
    if bool(fg.any()):
        iou = bbox_ciou_const_alpha(pred_bboxes[fg], target_bboxes[fg]).squeeze(-1)  # BboxLoss (:99-106)
        box_term = ((1.0 - iou) * weight[fg]).sum() / tss
        x1y1, x2y2 = target_bboxes.chunk(2, -1)
        t = torch.cat((anchor_points - x1y1, x2y2 - anchor_points), -1).clamp(0, REG_MAX - 1 - 0.01)[fg]  # bbox2dist
        tl = t.long()  # DFLoss (:73-88)
        tr = tl + 1
        wl = tr - t
        wr = 1 - wl
        pd = pred_distri.reshape(B, A, 4, REG_MAX)[fg].reshape(-1, REG_MAX)
        ce_l = F.cross_entropy(pd, tl.view(-1), reduction="none").view(tl.shape)
        ce_r = F.cross_entropy(pd, tr.view(-1), reduction="none").view(tl.shape)
        dfl_term = ((ce_l * wl + ce_r * wr).mean(-1) * weight[fg]).sum() / tss
    terms = torch.stack((box_term, cls_term, dfl_term)) * torch.tensor(gains, dtype=dtype, device=dev)
    return terms.sum() * B, terms


def given_assignment_grads(box_logits, cls_logits, shapes, strides, gt, fg, target_gt_idx, target_score,
                           target_scores_sum, gains=GAINS, dtype=torch.float64):
    """d(total) / d(box logits), d(total) / d(class logits) by torch autograd in ``dtype``, and the terms."""
    box = box_logits.detach().to(dtype).requires_grad_(True)
    cls = cls_logits.detach().to(dtype).requires_grad_(True)
    total, terms = given_assignment_loss(box, cls, shapes, strides, gt, fg, target_gt_idx, target_score,
                                         target_scores_sum, gains, dtype)
    gb, gc = torch.autograd.grad(total, (box, cls))
    return gb, gc, terms.detach()
