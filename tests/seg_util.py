"""Yardstick of the segmentation tests (test infrastructure; imports oracle/).

Plain-torch CPU restatements of Proto (U/nn/modules/block.py:87-104), Segment (U/nn/modules/head.py:224-271) and of
crop_mask, process_mask, process_mask_native and scale_masks (U/utils/ops.py:644-737), built on oracle.model's Conv /
Detect so that a2c2f_util.fuse_ folds them; builders of the two segmentation models on top of yolo11_util's baselines
(the oracle's parser knows Detect only: the head is swapped for the restated Segment before the weights are drawn);
the mask test inputs shared by the host and the GPU tests, and the rule masks are compared by.

The mask functions take a `dtype` for their fp64 legs and `threshold=False` to return the values the final `> 0` is
taken of.  Boxes stay fp32 in every leg and are scaled by the fp32 product torch computes (`bboxes[:, 0] *=
width_ratio` on an fp32 tensor): the indicator is a property of the call, not of the leg's precision.
"""

from __future__ import annotations

import copy

import torch
import torch.nn as nn
import torch.nn.functional as F

import oracle.model as om
import yolo11_util as U
from a2c2f_util import fuse_, leg_bound, legs  # noqa: F401 (re-exported)
from oracle.model import Conv

GOLDEN = U.GOLDEN
NEAR_ZERO = 2.0**-16   # |v64| <= NEAR_ZERO * S: the sign of such a pixel is not asserted
NEAR_ZERO_CAP = 1e-3   # the share of S > 0 pixels that may be near zero


class Proto(nn.Module):
    """block.py:87-104."""

    def __init__(self, c1, c_=256, c2=32):
        super().__init__()
        self.cv1 = Conv(c1, c_, k=3)
        self.upsample = nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True)
        self.cv2 = Conv(c_, c_, k=3)
        self.cv3 = Conv(c_, c2)

    def forward(self, x):
        return self.cv3(self.cv2(self.upsample(self.cv1(x))))


class Segment(om.Detect):
    """head.py:224-271 (inference, export False)."""

    def __init__(self, nc=80, nm=32, npr=256, ch=(), legacy=False):
        super().__init__(nc, ch, legacy=legacy)
        self.nm = nm
        self.npr = npr
        self.proto = Proto(ch[0], self.npr, self.nm)
        c4 = max(ch[0] // 4, self.nm)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nm, 1)) for x in ch)

    def forward(self, x):
        p = self.proto(x[0])
        bs = p.shape[0]
        mc = torch.cat([self.cv4[i](x[i]).view(bs, self.nm, -1) for i in range(self.nl)], 2)
        x = om.Detect.forward(self, x)
        if self.training:
            return x, mc, p
        return torch.cat([x[0], mc], 1), (x[1], mc, p)


# ----------------------------------------------------------------------------- the mask functions
def crop_mask(masks, boxes):
    """ops.py:644-658."""
    _, h, w = masks.shape
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    r = torch.arange(w, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, dtype=x1.dtype)[None, :, None]
    return masks * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


def scale_masks(masks, shape, padding=True):
    """ops.py:716-737."""
    mh, mw = masks.shape[2:]
    gain = min(mh / shape[0], mw / shape[1])
    pad = [mw - shape[1] * gain, mh - shape[0] * gain]
    if padding:
        pad[0] /= 2
        pad[1] /= 2
    top, left = (int(pad[1]), int(pad[0])) if padding else (0, 0)
    bottom, right = (int(mh - pad[1]), int(mw - pad[0]))
    masks = masks[..., top:bottom, left:right]
    return F.interpolate(masks, shape, mode="bilinear", align_corners=False)


def process_mask(protos, masks_in, bboxes, shape, upsample=False, dtype=torch.float32, threshold=True):
    """ops.py:661-693; protos [c, mh, mw], masks_in [n, c], bboxes [n, 4] fp32."""
    c, mh, mw = protos.shape
    ih, iw = shape
    masks = (masks_in.to(dtype) @ protos.float().to(dtype).view(c, -1)).view(-1, mh, mw)
    width_ratio = mw / iw
    height_ratio = mh / ih
    downsampled_bboxes = bboxes.float().clone()
    downsampled_bboxes[:, 0] *= width_ratio
    downsampled_bboxes[:, 2] *= width_ratio
    downsampled_bboxes[:, 3] *= height_ratio
    downsampled_bboxes[:, 1] *= height_ratio
    masks = crop_mask(masks, downsampled_bboxes.to(dtype))  # (an fp32 value is exact in fp64: the same indicator)
    if upsample:
        masks = F.interpolate(masks[None], shape, mode="bilinear", align_corners=False)[0]
    return masks.gt_(0.0) if threshold else masks


def process_mask_native(protos, masks_in, bboxes, shape, dtype=torch.float32, threshold=True):
    """ops.py:696-713."""
    c, mh, mw = protos.shape
    masks = (masks_in.to(dtype) @ protos.float().to(dtype).view(c, -1)).view(-1, mh, mw)
    masks = scale_masks(masks[None], shape)[0]
    masks = crop_mask(masks, bboxes.float().to(dtype))
    return masks.gt_(0.0) if threshold else masks


# ----------------------------------------------------------------------------- mask test inputs and the comparison rule
def mask_boxes(ih: int, iw: int) -> torch.Tensor:
    """Seven boxes in (ih, iw) pixels: edges exactly on the proto grid at ratio 1/4, reaching outside the image, zero
    area, the whole image, fractional, thin and tall, the bottom-right corner."""
    return torch.tensor([
        [32.0, 16.0, 64.0, 48.0],
        [-20.5, 10.2, iw + 30.0, ih * 0.6],
        [50.0, 30.0, 50.0, 30.0],
        [0.0, 0.0, float(iw), float(ih)],
        [10.3, 7.7, 25.9, 40.1],
        [iw * 0.5 + 0.4, 2.2, iw * 0.5 + 3.1, ih - 1.5],
        [iw - 17.3, ih - 21.8, iw - 0.2, ih - 0.4]], dtype=torch.float32)


# (form, mh, mw, target shape or None): process_mask upsample=True to 4x the grid, upsample=False, and
# process_mask_native through scale_masks' window to sizes that are no multiple of anything
MASK_FORMS = [("up", 24, 40, (96, 160)), ("up", 16, 16, (64, 64)), ("same", 24, 40, (96, 160)),
              ("same", 16, 16, (64, 64)), ("native", 24, 40, (75, 150)), ("native", 24, 40, (101, 127)),
              ("native", 16, 16, (200, 173))]
MASK_COUNTS = [(7, 0), (1, 7)]  # detections per image: 0, 1 and 7 all occur


def mask_inputs(seed: int, mh: int, mw: int, nm: int = 32, half: bool = False):
    """N(0, 1) prototypes [2, mh, mw, nm] (NHWC; rounded to fp16 when half) and coefficients [2, 7, nm]."""
    g = torch.Generator().manual_seed(seed)
    proto = torch.randn(2, mh, mw, nm, generator=g)
    coef = torch.randn(2, 7, nm, generator=g)
    return (proto.half() if half else proto), coef


def mask_reference(form, proto, coef, boxes, counts, shape):
    """Per image the restatement's fp64 values and S, the same pipeline on |coef|, |proto|: lists of [k, H, W] fp64
    tensors (k = counts[b]; an empty tensor for 0).  `shape` is the input image's (h, w) for "up" / "same" (the boxes'
    frame), the target for "native"."""
    vs, ss = [], []
    for b, k in enumerate(counts):
        if k == 0:  # (F.interpolate refuses an empty batch)
            vs.append(torch.zeros(0, 1, 1, dtype=torch.float64))
            ss.append(torch.zeros(0, 1, 1, dtype=torch.float64))
            continue
        p = proto[b].permute(2, 0, 1).float()
        c, bx = coef[b, :k], boxes[:k]
        out = []
        for pp, cc in ((p, c), (p.abs(), c.abs())):
            if form == "native":
                out.append(process_mask_native(pp, cc, bx, shape, dtype=torch.float64, threshold=False))
            else:
                out.append(process_mask(pp, cc, bx, shape, upsample=form == "up", dtype=torch.float64,
                                        threshold=False))
        vs.append(out[0])
        ss.append(out[1])
    return vs, ss


def mask_leg32(form, proto, coef, boxes, counts, shape):
    """The restatement's own fp32 leg, thresholded: per image [k, H, W] 0 / 1."""
    outs = []
    for b, k in enumerate(counts):
        p = proto[b].permute(2, 0, 1).float()
        if form == "native":
            outs.append(process_mask_native(p, coef[b, :k], boxes[:k], shape))
        else:
            outs.append(process_mask(p, coef[b, :k], boxes[:k], shape, upsample=form == "up"))
    return outs


def mask_check(got, v64, S):
    """The rule one image's masks are compared by.  got: 0 / 1 values [k, H, W]; v64, S: mask_reference's.  Returns
    (wrong, near, pos): pixels that break the rule -- nonzero where S == 0, or different from v64 > 0 outside the
    near-zero set |v64| <= 2^-16 S -- the size of the near-zero set, and the number of S > 0 pixels."""
    got = got.double()
    pos = S > 0
    near = pos & (v64.abs() <= NEAR_ZERO * S)
    wrong = (~pos & (got != 0)) | (pos & ~near & (got != (v64 > 0).double()))
    return int(wrong.sum()), int(near.sum()), int(pos.sum())


# ----------------------------------------------------------------------------- models
FAMILIES = U.FAMILIES


def build_oracle(family: str, scale: str = "n", nc: int = 3, nm: int = 32, npr: int = 256):
    """The restated segmentation model (eval, unfused) under torch.manual_seed(0) with trained-like BN: the detection
    baseline of yolo11_util with its head rebuilt as Segment (npr scaled as parse_model scales it,
    U/nn/tasks.py:1109-1110) before the weights are drawn."""
    from ydbl.utils.synthetic import trained_like_

    U.register()
    torch.manual_seed(0)
    cfg = U.baseline_cfg(family, scale, nc)
    o = om.DetectionModel(cfg, stride_probe=False)
    head = o.model[-1]
    ch = [seq[0].conv.in_channels for seq in head.cv2]
    _, width, max_channels = cfg["scales"][scale]
    new = Segment(head.nc, nm, om.make_divisible(min(npr, max_channels) * width, 8), ch, legacy=FAMILIES[family])
    new.i, new.f, new.type, new.n_ = head.i, head.f, "Segment", head.n_
    new.stride = head.stride
    new.bias_init()
    for mod in new.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.eps, mod.momentum = 1e-3, 0.03
    o.model[-1] = new
    o.eval()
    return trained_like_(o, 0)


@torch.no_grad()
def sensitize_(o: nn.Module, x: torch.Tensor) -> nn.Module:
    """Make a restated model's output depend on its input.  With init weights the signal of an image dies within a few
    layers under the trained-like BN statistics, and every image gets the same prediction to six digits; a test that
    needs one image with detections and one without cannot be built on that.  One forward pass on x rescales every
    Conv's weight, in execution order, so that its pre-BN output has unit standard deviation on x (the output is
    rescaled on the way, so the next layer sees what it will see afterwards).  The final 1x1 convs of the heads and
    Proto's ConvTranspose2d keep their init."""
    def hook(mod, inp, out):
        s = out.std().item()
        if s > 0:
            mod.weight *= 1.0 / s
            return out * (1.0 / s)

    hooks = [m.conv.register_forward_hook(hook) for m in o.modules() if isinstance(m, Conv)]
    o(x)
    for h in hooks:
        h.remove()
    return o


def build_pair(family: str, scale: str = "n", nc: int = 3, x: torch.Tensor | None = None):
    """(product YOLO, fused fp32 restatement) with identical weights, copied by load_state_dict(strict=True); x: the
    batch sensitize_() scales the weights on first."""
    from ydbl import YOLO

    o = build_oracle(family, scale, nc)
    if x is not None:
        sensitize_(o, x)
    p = YOLO(str(GOLDEN / f"{family}{scale}-seg.json"), nc=nc)
    p.model.load_state_dict(o.state_dict(), strict=True)
    return p, copy.deepcopy(o).fuse()
