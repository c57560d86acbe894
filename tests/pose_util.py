"""Yardstick of the pose tests (test infrastructure; imports oracle/).

Plain-torch CPU restatements of Pose (U/nn/modules/head.py:328-401, inference with export False), of scale_coords /
clip_coords (U/utils/ops.py:341-358, :740-772), kpt_iou (U/utils/metrics.py:156-175) and of the keypoint half of
PoseValidator (U/models/yolo/pose/val.py:106-197) on top of oracle.metrics.match_predictions; builders of the two pose
models on top of yolo11_util's baselines, as seg_util builds the segmentation ones (the oracle's parser knows Detect
only: the head is swapped for the restated Pose before the weights are drawn).
"""

from __future__ import annotations

import copy

import numpy as np
import torch
import torch.nn as nn

import oracle.model as om
import yolo11_util as U
from oracle.metrics import IOUV, match_predictions
from oracle.model import Conv
from seg_util import sensitize_  # noqa: F401 (re-exported)

GOLDEN = U.GOLDEN
FAMILIES = U.FAMILIES

# the COCO keypoint sigmas (metrics.py:15-18)
OKS_SIGMA = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


class Pose(om.Detect):
    """head.py:328-401 (inference, export False)."""

    def __init__(self, nc=80, kpt_shape=(17, 3), ch=(), legacy=False):
        super().__init__(nc, ch, legacy=legacy)
        self.kpt_shape = kpt_shape
        self.nk = kpt_shape[0] * kpt_shape[1]
        c4 = max(ch[0] // 4, self.nk)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nk, 1)) for x in ch)

    def forward(self, x):
        bs = x[0].shape[0]
        hws = [tuple(t.shape[2:]) for t in x]
        kpt = torch.cat([self.cv4[i](x[i]).view(bs, self.nk, -1) for i in range(self.nl)], -1)
        x = om.Detect.forward(self, x)
        if self.training:
            return x, kpt
        return torch.cat([x[0], kpts_decode(kpt, hws, self.stride.tolist(), self.kpt_shape[1])], 1), (x[1], kpt)


def anchor_grid(hws, strides, dtype=torch.float32):
    """(gx [A], gy [A], stride [A]): the anchors' grid cells (make_anchors' points minus 0.5) level after level,
    row-major, and each anchor's stride."""
    gx, gy, st = [], [], []
    for (h, w), s in zip(hws, strides):
        yy, xx = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing="ij")
        gx.append(xx.reshape(-1))
        gy.append(yy.reshape(-1))
        st.append(torch.full((h * w,), float(s), dtype=dtype))
    return torch.cat(gx), torch.cat(gy), torch.cat(st)


def kpts_decode(kpt, hws, strides, ndim):
    """head.py:396-401 on kpt [B, nk, A], in kpt's dtype."""
    gx, gy, st = anchor_grid(hws, strides, kpt.dtype)
    y = kpt.clone()
    if ndim == 3:
        y[:, 2::3] = y[:, 2::3].sigmoid()
    y[:, 0::ndim] = (y[:, 0::ndim] * 2.0 + gx) * st
    y[:, 1::ndim] = (y[:, 1::ndim] * 2.0 + gy) * st
    return y


def decode_rows(raw, anchors, hws, strides, ndim, dtype=torch.float32):
    """The decode of single anchors: raw [k, K * ndim] (the stored values of the anchors `anchors` [k], indices on
    the concatenated anchor axis) -> [k, K, ndim] in `dtype`; the visibility through torch's sigmoid."""
    gx, gy, st = anchor_grid(hws, strides, dtype)
    a = torch.as_tensor(anchors).long()
    v = raw.to(dtype).reshape(len(a), -1, ndim).clone()
    v[..., 0] = (v[..., 0] * 2.0 + gx[a][:, None]) * st[a][:, None]
    v[..., 1] = (v[..., 1] * 2.0 + gy[a][:, None]) * st[a][:, None]
    if ndim == 3:
        v[..., 2] = v[..., 2].sigmoid()
    return v


# ----------------------------------------------------------------------------- coordinates
def clip_coords(coords, shape):
    """ops.py:341-358."""
    if isinstance(coords, torch.Tensor):
        coords[..., 0] = coords[..., 0].clamp(0, shape[1])
        coords[..., 1] = coords[..., 1].clamp(0, shape[0])
    else:
        coords[..., 0] = coords[..., 0].clip(0, shape[1])
        coords[..., 1] = coords[..., 1].clip(0, shape[0])
    return coords


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None, normalize=False, padding=True):
    """ops.py:740-772."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    if padding:
        coords[..., 0] -= pad[0]
        coords[..., 1] -= pad[1]
    coords[..., 0] /= gain
    coords[..., 1] /= gain
    coords = clip_coords(coords, img0_shape)
    if normalize:
        coords[..., 0] /= img0_shape[1]
        coords[..., 1] /= img0_shape[0]
    return coords


# ----------------------------------------------------------------------------- OKS and the matching
def kpt_iou(kpt1, kpt2, area, sigma, eps=1e-7):
    """metrics.py:156-175; in the dtype of kpt1 (fp64 for the yardstick)."""
    d = (kpt1[:, None, :, 0] - kpt2[..., 0]).pow(2) + (kpt1[:, None, :, 1] - kpt2[..., 1]).pow(2)
    sigma = torch.tensor(np.asarray(sigma), dtype=kpt1.dtype)
    kpt_mask = kpt1[..., 2] != 0
    e = d / ((2 * sigma).pow(2) * (area[:, None, None] + eps) * 2)
    return ((-e).exp() * kpt_mask[:, None]).sum(-1) / (kpt_mask.sum(-1)[:, None] + eps)


def gt_area(boxes):
    """pose/val.py:192: xyxy2xywh(bbox)[:, 2:].prod(1) * 0.53."""
    return ((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])) * 0.53


def oks_ref(pred_kpts, counts, gt_kpts, gt_box, bidx, sigma, dtype=torch.float64):
    """Per image with labels and predictions: (image, OKS [nl, npr]) in `dtype`, labels in their order within the
    image."""
    out = []
    bidx = torch.as_tensor(bidx).reshape(-1).long()
    for si in range(pred_kpts.shape[0]):
        sel = bidx == si
        npr = int(counts[si])
        if npr == 0 or not sel.any():
            continue
        g, bx = gt_kpts[sel].to(dtype), gt_box[sel].to(dtype)
        out.append((si, kpt_iou(g, pred_kpts[si, :npr].to(dtype), gt_area(bx), sigma)))
    return out


def tp_p_ref(det, counts, pred_kpts, gt_kpts, gt_box, gt_cls, bidx, sigma, single_cls=False, iouv=IOUV):
    """update_metrics' tp_p blocks (pose/val.py:106-145) for a batch on the CPU, in the validator's order, from the
    fp32 restatement of kpt_iou."""
    blocks = []
    bidx = torch.as_tensor(bidx).reshape(-1).long()
    gt_cls = torch.as_tensor(gt_cls).reshape(-1).float()
    for si in range(det.shape[0]):
        npr = int(counts[si])
        sel = bidx == si
        cls = gt_cls[sel]
        nl = len(cls)
        if npr == 0:
            if nl:
                blocks.append(torch.zeros(0, len(iouv), dtype=torch.bool))
            continue
        pc = det[si, :npr, 5].clone()
        if single_cls:
            pc[:] = 0
        if nl == 0:
            blocks.append(torch.zeros(npr, len(iouv), dtype=torch.bool))
            continue
        iou = kpt_iou(gt_kpts[sel].float(), pred_kpts[si, :npr].float(), gt_area(gt_box[sel].float()), sigma)
        blocks.append(match_predictions(pc, cls, iou, iouv))
    return blocks


def threshold_margin(oks_list, gt_cls, bidx, det, counts, iouv=IOUV) -> float:
    """The smallest distance of a same-class (label, detection) OKS value from any threshold of iouv."""
    bidx = torch.as_tensor(bidx).reshape(-1).long()
    gt_cls = torch.as_tensor(gt_cls).reshape(-1).float()
    best = float("inf")
    thr = torch.as_tensor(iouv).double()
    for si, oks in oks_list:
        same = gt_cls[bidx == si][:, None] == det[si, : int(counts[si]), 5][None]
        v = oks.double()[same]
        if v.numel():
            best = min(best, float((v[:, None] - thr[None]).abs().min()))
    return best


# ----------------------------------------------------------------------------- models
def build_oracle(family: str, scale: str = "n", nc: int = 1, kpt_shape=(17, 3)):
    """The restated pose model (eval, unfused) under torch.manual_seed(0) with trained-like BN: the detection baseline
    of yolo11_util with its head rebuilt as Pose before the weights are drawn."""
    from ydbl.utils.synthetic import trained_like_

    U.register()
    torch.manual_seed(0)
    cfg = U.baseline_cfg(family, scale, nc)
    o = om.DetectionModel(cfg, stride_probe=False)
    head = o.model[-1]
    ch = [seq[0].conv.in_channels for seq in head.cv2]
    new = Pose(head.nc, tuple(kpt_shape), ch, legacy=FAMILIES[family])
    new.i, new.f, new.type, new.n_ = head.i, head.f, "Pose", head.n_
    new.stride = head.stride
    new.bias_init()
    for mod in new.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.eps, mod.momentum = 1e-3, 0.03
    o.model[-1] = new
    o.eval()
    return trained_like_(o, 0)


def build_pair(family: str, scale: str = "n", nc: int = 1, x: torch.Tensor | None = None, kpt_shape=(17, 3)):
    """(product YOLO, fused fp32 restatement) with identical weights, copied by load_state_dict(strict=True); x: the
    batch sensitize_() scales the weights on first."""
    from a2c2f_util import fuse_  # noqa: F401
    from ydbl import YOLO

    o = build_oracle(family, scale, nc, kpt_shape)
    if x is not None:
        sensitize_(o, x)
    p = YOLO(str(GOLDEN / f"{family}{scale}-pose.json"), nc=nc, kpt_shape=list(kpt_shape))
    p.model.load_state_dict(o.state_dict(), strict=True)
    return p, copy.deepcopy(o).fuse()
