"""Yardstick of the YOLO11 / YOLOv8 baseline tests (test infrastructure; imports oracle/).

Plain-torch CPU restatements of SPPF (U/nn/modules/block.py:179-198), C3k2 / C3k (:734-753), Attention (:896-930),
PSABlock (:955-967) and C2PSA (:1038-1052), built on oracle.model's Conv / Bottleneck / C2f / C3 so that the oracle's
fuse() folds them; builders of the two baseline models through oracle.model.DetectionModel with a dict cfg; and the
peakedness tools of the 128-channel-per-head attention.  The classes are registered in oracle.model's tables
in-process; no file under oracle/ is edited.  leg_bound, legs, fuse_ and the nn.Upsample wrapper come from a2c2f_util.
"""

from __future__ import annotations

import copy
import json
from pathlib import Path

import torch
import torch.nn as nn

import oracle.model as om
from a2c2f_util import Upsample, fuse_, leg_bound, legs  # noqa: F401 (re-exported)
from oracle.model import C3, Bottleneck, C2f, Conv

GOLDEN = Path(__file__).resolve().parent / "golden"
KD, HD = 32, 64  # key_dim and head_dim of every stock C2PSA


class SPPF(nn.Module):
    """block.py:179-198: cv1, three chained max-pools, cv2 over the four maps."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)

    def forward(self, x):
        y = [self.cv1(x)]
        for _ in range(3):
            y.append(self.m(y[-1]))
        return self.cv2(torch.cat(y, 1))


class C3k(C3):
    """block.py:745-753."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, k=3):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=(k, k), e=1.0) for _ in range(n)))


class C3k2(C2f):
    """block.py:734-742."""

    def __init__(self, c1, c2, n=1, c3k=False, e=0.5, g=1, shortcut=True):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(
            C3k(self.c, self.c, 2, shortcut, g) if c3k else Bottleneck(self.c, self.c, shortcut, g) for _ in range(n))


class Attention(nn.Module):
    """block.py:896-930."""

    def __init__(self, dim, num_heads=8, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim**-0.5
        self.qkv = Conv(dim, dim + 2 * self.key_dim * num_heads, 1, act=False)
        self.proj = Conv(dim, dim, 1, act=False)
        self.pe = Conv(dim, dim, 3, 1, g=dim, act=False)

    def split(self, qkv):
        """q, k [B, heads, key_dim, N] and v [B, heads, head_dim, N] of qkv [B, heads*(2kd+hd), H, W] (:922-924)."""
        B, _, H, W = qkv.shape
        per = 2 * self.key_dim + self.head_dim
        return qkv.reshape(B, self.num_heads, per, H * W).split([self.key_dim, self.key_dim, self.head_dim], dim=2)

    def core(self, qkv):
        """:919-928 without the convs: qkv [B, heads*(2kd+hd), H, W] -> (attention output, v), both [B, C, H, W]."""
        B, _, H, W = qkv.shape
        q, k, v = self.split(qkv)
        p = ((q.transpose(-2, -1) @ k) * self.scale).softmax(dim=-1)
        y = v @ p.transpose(-2, -1)
        C = self.num_heads * self.head_dim
        return y.reshape(B, C, H, W), v.reshape(B, C, H, W)

    def forward(self, x):
        y, v = self.core(self.qkv(x))
        return self.proj(y + self.pe(v))


class PSABlock(nn.Module):
    """block.py:955-967."""

    def __init__(self, c, attn_ratio=0.5, num_heads=4, shortcut=True):
        super().__init__()
        self.attn = Attention(c, attn_ratio=attn_ratio, num_heads=num_heads)
        self.ffn = nn.Sequential(Conv(c, c * 2, 1), Conv(c * 2, c, 1, act=False))
        self.add = shortcut

    def forward(self, x):
        x = x + self.attn(x) if self.add else self.attn(x)
        return x + self.ffn(x) if self.add else self.ffn(x)


class C2PSA(nn.Module):
    """block.py:1038-1052."""

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.m = nn.Sequential(*(PSABlock(self.c, attn_ratio=0.5, num_heads=self.c // 64) for _ in range(n)))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), dim=1)
        return self.cv2(torch.cat((a, self.m(b)), 1))


def register():
    """The new classes and nn.Upsample in the oracle's parser tables (in-process)."""
    for cls in (SPPF, C3k, C3k2, Attention, PSABlock, C2PSA):
        om._CLASSES[cls.__name__] = cls
    om._CLASSES["nn.Upsample"] = Upsample
    om._C1C2.update({"SPPF", "C3k2", "C2PSA"})
    om._REPEAT_INSERT.update({"C3k2", "C2PSA"})


FAMILIES = {"yolo11": False, "yolov8": True}  # family -> Detect.legacy (U/nn/tasks.py:1084-1085: C3k2 clears it)


def baseline_cfg(family: str, scale: str, nc: int | None = None) -> dict:
    d = json.loads((GOLDEN / f"{family}.json").read_text())
    d["scale"] = scale
    if nc:
        d["nc"] = nc
    return d


def build_oracle(family: str, scale: str, nc: int = 3):
    """The restated baseline model (eval, unfused) under torch.manual_seed(0) with trained-like BN.  The oracle's
    parser does not know that C3k2 clears `legacy`, so for yolo11 its head is rebuilt in the legacy=False form (before
    the weights are drawn)."""
    from ydbl.utils.synthetic import trained_like_

    register()
    torch.manual_seed(0)
    o = om.DetectionModel(baseline_cfg(family, scale, nc), stride_probe=False)
    head = o.model[-1]
    if head.legacy != FAMILIES[family]:
        ch = [seq[0].conv.in_channels for seq in head.cv2]
        new = om.Detect(head.nc, ch, legacy=FAMILIES[family])
        new.i, new.f, new.type, new.n_ = head.i, head.f, head.type, head.n_
        new.stride = head.stride
        new.bias_init()
        for mod in new.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.eps, mod.momentum = 1e-3, 0.03
        o.model[-1] = new
    o.eval()
    assert o.model[-1].legacy is FAMILIES[family]
    return trained_like_(o, 0)


def build_pair(family: str, scale: str, nc: int = 3):
    """(product YOLO, fused fp32 restatement) with identical weights, copied by load_state_dict(strict=True)."""
    from ydbl import YOLO

    o = build_oracle(family, scale, nc)
    p = YOLO(str(GOLDEN / f"{family}{scale}.json"), nc=nc)
    p.model.load_state_dict(o.state_dict(), strict=True)
    return p, copy.deepcopy(o).fuse()


# ----------------------------------------------------------------------------- attention references and peakedness
def psa_ref(qkv_nhwc: torch.Tensor, heads: int, dtype):
    """Attention's core on an NHWC qkv [n,h,w,heads*128] by torch-CPU in `dtype` -> (y, v) NHWC [n,h,w,heads*64].
    dtype float16: half q^T k, half softmax, half P v, as the reference's half=True path runs it."""
    a = Attention(heads * HD, heads, 0.5)
    y, v = a.core(qkv_nhwc.permute(0, 3, 1, 2).to(dtype))
    return y.permute(0, 2, 3, 1).contiguous(), v.permute(0, 2, 3, 1).contiguous()


def peakedness(qkv_nhwc: torch.Tensor, heads: int) -> float:
    """Mean over query rows of the row-maximum softmax probability, in fp64."""
    a = Attention(heads * HD, heads, 0.5)
    q, k, _ = a.split(qkv_nhwc.permute(0, 3, 1, 2).double())
    return ((q.transpose(-2, -1) @ k) * a.scale).softmax(-1).amax(-1).mean().item()


@torch.no_grad()
def attn_peaks(m: nn.Module, x: torch.Tensor) -> list[float]:
    """peakedness() of every Attention inside the restated module m on input x, in fp64 after BN folding."""
    f = fuse_(copy.deepcopy(m).eval()).double()
    got, hooks = [], []
    for a in f.modules():
        if isinstance(a, Attention):
            hooks.append(a.qkv.register_forward_hook(
                lambda mod, inp, out, a=a: got.append(peakedness(out.permute(0, 2, 3, 1), a.num_heads))))
    f(x.double())
    for h in hooks:
        h.remove()
    return got


def _rows(a: Attention):
    """qkv's weight as [heads, 128, cin]: rows 0..63 of a head are q | k, rows 64..127 v."""
    return a.qkv.conv.weight.view(a.num_heads, 2 * a.key_dim + a.head_dim, -1)


@torch.no_grad()
def sharpen_(m: nn.Module, x: torch.Tensor, floor: float = 0.2) -> list[float]:
    """Make the attention of a restated module matter on input x: v rows of every qkv and every proj x 8 (the
    attention branch is not lost under the residual), q / k rows scaled until every Attention's peakedness is
    >= floor.  Returns the final peakedness values.

    The search lands every Attention just above the floor, from either side and in forward order (an upstream block
    changes its successor's input): the q / k step is 2^(1/8) (scores x 2^(1/4) per round); an Attention that starts
    above the floor -- the second block of a C2PSA, whose input the first block's x 8 x 8 has already blown up -- is
    first scaled down until it is below, then up until it is at or above.  A softmax far above the floor (doubling q and k quadruples the scores and landed at 0.57-0.9
    with scores of +-33) multiplies the fp32 rounding of the 1x1 conv that produces q and k by the score magnitude:
    the module bound then measures the summation order of that conv (a kernel these tests do not add), not the
    attention."""
    attns = [a for a in m.modules() if isinstance(a, Attention)]
    for a in attns:
        _rows(a)[:, 2 * a.key_dim:] *= 8.0
        a.proj.conv.weight *= 8.0
    step = 2.0**0.125
    for i, a in enumerate(attns):  # in forward order: an Attention's input is final before it is tuned
        qk = _rows(a)[:, :2 * a.key_dim]
        for _ in range(160):  # down until below the floor
            if attn_peaks(m, x)[i] < floor:
                break
            qk /= step
        for _ in range(160):  # up: stops at the first round at or above the floor
            if attn_peaks(m, x)[i] >= floor:
                break
            qk *= step
    peaks = attn_peaks(m, x)
    if min(peaks) < floor:
        raise AssertionError(f"could not reach peakedness {floor}: {peaks}")
    return peaks
