"""Test-time augmentation as the reference computes it, restated with torch-CPU ops for the tests
(test infrastructure; the oracle's per-pass forward comes from oracle/model.py).

An input batch x [B,3,H,W] in 0..1 goes through the network three times: as it is, mirrored left-right and shrunk
to 0.83, and shrunk to 0.67.  Shrinking is a bilinear resize without corner alignment to the truncated size,
followed by constant 0.447 padding on the right and bottom up to the next multiple of the largest stride above
H * ratio (not above the truncated size).  Each pass's decoded boxes are divided by its ratio, the mirrored pass's
centre x is reflected about the original width, the first pass gives up its coarsest level's share of the anchor
axis at the end, the last pass its finest level's share at the start, and what remains is laid side by side in
pass order for one NMS.
"""

from __future__ import annotations

import copy
import math

import torch
import torch.nn.functional as F

PASSES = ((1.0, False), (0.83, True), (0.67, False))  # (ratio, mirrored)
PAD_VALUE = 0.447


def pass_sizes(h, w, ratio, gs=32):
    """((resized h, w), (padded h, w)) of one pass."""
    if ratio == 1.0:
        return (h, w), (h, w)
    return (int(h * ratio), int(w * ratio)), (math.ceil(h * ratio / gs) * gs, math.ceil(w * ratio / gs) * gs)


def expected_passes(h, w, strides=(8, 16, 32)):
    """The rows ydbl.engine.session.augment_passes must return, from the formulas written out."""
    nl = len(strides)
    g = sum(4 ** k for k in range(nl))  # 1 + 4 + 16 for three levels
    rows, pos = [], 0
    for i, (ratio, flip) in enumerate(PASSES):
        s, p = pass_sizes(h, w, ratio, max(strides))
        A = sum((p[0] // st) * (p[1] // st) for st in strides)
        lo, hi = 0, A
        if i == 0:
            hi = A - A // g
        if i == len(PASSES) - 1:
            lo = (A // g) * 4 ** (nl - 1)
        rows.append((ratio, flip, s, p, A, lo, hi, pos))
        pos += hi - lo
    return rows


def scale_img_cpu(x, ratio, flip=False, gs=32):
    """One pass's network input from x (any float dtype), on the CPU."""
    if flip:
        x = x.flip(3)
    if ratio == 1.0:
        return x
    h, w = x.shape[2:]
    (sh, sw), (hp, wp) = pass_sizes(h, w, ratio, gs)
    y = F.interpolate(x, size=(sh, sw), mode="bilinear", align_corners=False)
    return F.pad(y, [0, wp - sw, 0, hp - sh], value=PAD_VALUE)


def merge_passes(ys, width, nl=3):
    """ys: the three passes' decoded predictions [B, 4+nc, A_i] (not modified) -> the merged [B, 4+nc, A_tot]."""
    g = sum(4 ** k for k in range(nl))
    out = []
    for i, (y, (ratio, flip)) in enumerate(zip(ys, PASSES)):
        y = y.clone()
        y[:, :4] /= ratio
        if flip:
            y[:, 0] = width - y[:, 0]
        A = y.shape[-1]
        if i == 0:
            y = y[..., : A - A // g]
        if i == len(PASSES) - 1:
            y = y[..., (A // g) * 4 ** (nl - 1):]
        out.append(y)
    return torch.cat(out, -1)


@torch.inference_mode()
def oracle_augment(o, x, legs=("fp64", "fp32")):
    """The merged prediction of the fused oracle `o` in each precision: every step of the pipeline (resize
    included) in that precision."""
    out = {}
    for leg in legs:
        m, xin = (copy.deepcopy(o).double(), x.double()) if leg == "fp64" else (o, x.float())
        ys = [m(scale_img_cpu(xin, r, f))[0] for r, f in PASSES]
        out[leg] = merge_passes(ys, x.shape[3])
    return out


def blob_batch(n, h, w, seed):
    """n blob images of (h, w): the top-left corner of square ones."""
    from ydbl.utils.synthetic import blob_images

    return blob_images(n, max(h, w), seed=seed)[:, :, :h, :w].contiguous()
