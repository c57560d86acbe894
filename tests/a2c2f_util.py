"""Yardstick of the YOLOv13 baseline tests (test infrastructure; imports oracle/).

A plain-torch CPU restatement of AAttn / ABlock / A2C2f (U/nn/modules/block.py:1187-1406), built on
oracle.model.Conv so that the oracle's fuse() folds it, a thin nn.Upsample wrapper, a builder of the baseline
model through oracle.model.DetectionModel with a dict cfg, and the leg-relative bounds of the attention tests.
The two classes are registered in oracle.model's tables in-process; no file under oracle/ is edited.
"""

from __future__ import annotations

import copy
import json
from pathlib import Path

import torch
import torch.nn as nn

import oracle.model as om
from oracle.model import Conv

GOLDEN = Path(__file__).resolve().parent / "golden"
CFG = GOLDEN / "yolov13.json"


class AAttn(nn.Module):
    """block.py:1187-1264."""

    def __init__(self, dim, num_heads, area=1):
        super().__init__()
        self.area = area
        self.num_heads = num_heads
        self.head_dim = head_dim = dim // num_heads
        all_head_dim = head_dim * self.num_heads
        self.qkv = Conv(dim, all_head_dim * 3, 1, act=False)
        self.proj = Conv(all_head_dim, dim, 1, act=False)
        self.pe = Conv(all_head_dim, dim, 7, 1, 3, g=dim, act=False)

    def split(self, qkv, B, C, N):
        """The per-chunk q, k, v [B*area, heads, head_dim, N/area] of block.py:1243-1254 from qkv [B, 3C, H, W]."""
        qkv = qkv.flatten(2).transpose(1, 2)
        if self.area > 1:
            qkv = qkv.reshape(B * self.area, N // self.area, C * 3)
            B, N, _ = qkv.shape
        return (qkv.view(B, N, self.num_heads, self.head_dim * 3).permute(0, 2, 3, 1)
                .split([self.head_dim, self.head_dim, self.head_dim], dim=2))

    def core(self, qkv):
        """block.py:1243-1270: qkv [B, 3C, H, W] -> (attention output, v) as [B, C, H, W]."""
        B, C3, H, W = qkv.shape
        C, N = C3 // 3, H * W
        q, k, v = self.split(qkv, B, C, N)
        attn = (q.transpose(-2, -1) @ k) * (self.head_dim**-0.5)
        attn = attn.softmax(dim=-1)
        x = v @ attn.transpose(-2, -1)
        x = x.permute(0, 3, 1, 2)
        v = v.permute(0, 3, 1, 2)
        if self.area > 1:
            x = x.reshape(B, N, C)
            v = v.reshape(B, N, C)
        x = x.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
        v = v.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
        return x, v

    def forward(self, x):
        x, v = self.core(self.qkv(x))
        x = x + self.pe(v)
        return self.proj(x)


class ABlock(nn.Module):
    """block.py:1268-1322."""

    def __init__(self, dim, num_heads, mlp_ratio=1.2, area=1):
        super().__init__()
        self.attn = AAttn(dim, num_heads=num_heads, area=area)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(Conv(dim, mlp_hidden_dim, 1), Conv(mlp_hidden_dim, dim, 1, act=False))
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Conv2d):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)

    def forward(self, x):
        x = x + self.attn(x)
        return x + self.mlp(x)


class A2C2f(nn.Module):
    """block.py:1325-1406 (a2=True only: no v13 config uses the C3k form)."""

    def __init__(self, c1, c2, n=1, a2=True, area=1, residual=False, mlp_ratio=2.0, e=0.5, g=1, shortcut=True):
        super().__init__()
        assert a2
        c_ = int(c2 * e)
        assert c_ % 32 == 0, "Dimension of ABlock must be a multiple of 32."
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv((1 + n) * c_, c2, 1)
        self.gamma = nn.Parameter(0.01 * torch.ones(c2), requires_grad=True) if a2 and residual else None
        self.m = nn.ModuleList(
            nn.Sequential(*(ABlock(c_, c_ // 32, mlp_ratio, area) for _ in range(2))) for _ in range(n))

    def forward(self, x):
        y = [self.cv1(x)]
        y.extend(m(y[-1]) for m in self.m)
        y = self.cv2(torch.cat(y, 1))
        if self.gamma is not None:
            return x + self.gamma.view(-1, self.gamma.shape[0], 1, 1) * y
        return y


class Upsample(nn.Upsample):
    """nn.Upsample as the YAML layer 'nn.Upsample'."""


def register():
    """A2C2f and nn.Upsample in the oracle's parser tables (in-process)."""
    om._CLASSES["A2C2f"] = A2C2f
    om._CLASSES["nn.Upsample"] = Upsample
    om._C1C2.add("A2C2f")
    om._REPEAT_INSERT.add("A2C2f")


def baseline_cfg(scale: str, nc: int | None = None) -> dict:
    """tests/golden/yolov13.json as the dict cfg of oracle.model.DetectionModel at `scale`; for l / x the A2C2f
    argument lists get the reference's scale rule (True, 1.5: U/nn/tasks.py:1087-1091), which the oracle's
    parser does not have."""
    d = json.loads(CFG.read_text())
    d["scale"] = scale
    if nc:
        d["nc"] = nc
    if scale in "lx":
        for layer in d["backbone"] + d["head"]:
            if layer[2] == "A2C2f":
                layer[3] = [*layer[3], True, 1.5]
    return d


def build_oracle(scale: str, nc: int = 3):
    """The restated baseline model (eval, unfused) under torch.manual_seed(0) with trained-like BN / gates."""
    from ydbl.utils.synthetic import trained_like_

    register()
    torch.manual_seed(0)
    o = om.DetectionModel(baseline_cfg(scale, nc), stride_probe=False).eval()
    # the A2C2f rule of U/nn/tasks.py:1088 (legacy = False) is not in the oracle's parser either: DSC3k2 and
    # HyperACE set it before Detect is built in this config, so the head already has the legacy=False form
    assert o.model[-1].legacy is False
    return trained_like_(o, 0)


def build_pair(scale: str, nc: int = 3):
    """(product YOLO, fused fp32 restatement) with identical weights, copied by load_state_dict(strict=True)."""
    from ydbl import YOLO

    o = build_oracle(scale, nc)
    p = YOLO(str(GOLDEN / f"yolov13{scale}.json"), nc=nc)
    p.model.load_state_dict(o.state_dict(), strict=True)
    return p, copy.deepcopy(o).fuse()


# ----------------------------------------------------------------------------- attention references and bounds
def attn_ref(qkv_nhwc: torch.Tensor, heads: int, area: int, dtype) -> torch.Tensor:
    """AAttn's core on an NHWC qkv [n,h,w,3C] evaluated by torch-CPU in `dtype` -> y NHWC [n,h,w,C] (dtype).
    dtype float16: half q^T k, half softmax, half P v, as the reference's half=True path runs it."""
    a = AAttn(heads * 32, heads, area)
    y, _ = a.core(qkv_nhwc.permute(0, 3, 1, 2).to(dtype))
    return y.permute(0, 2, 3, 1).contiguous()


def peakedness(qkv_nhwc: torch.Tensor, heads: int, area: int) -> float:
    """Mean over query rows of the row-maximum softmax probability, in fp64."""
    a = AAttn(heads * 32, heads, area)
    n, h, w, c3 = qkv_nhwc.shape
    q, k, _ = a.split(qkv_nhwc.permute(0, 3, 1, 2).double(), n, c3 // 3, h * w)
    p = ((q.transpose(-2, -1) @ k) * 32**-0.5).softmax(-1)
    return p.amax(-1).mean().item()


def leg_bound(y_leg: torch.Tensor, y64: torch.Tensor, half: bool, factor: float = 2.0) -> float:
    """The parity_util convention for one tensor: `factor` x the max deviation from fp64 of the torch-CPU leg of
    the same precision + one unit of roundoff of max|y| (2^-23 fp32, 2^-10 fp16)."""
    e = (y_leg.double() - y64).abs().max().item()
    return factor * e + y64.abs().max().item() * (2.0**-10 if half else 2.0**-23)


# ----------------------------------------------------------------------------- module-level helpers
def fuse_(m: nn.Module) -> nn.Module:
    """Fold BN into every oracle Conv of a stand-alone module (what DetectionModel.fuse does for a model)."""
    for c in m.modules():
        if isinstance(c, Conv) and hasattr(c, "bn"):
            c.conv = om.fuse_conv_and_bn(c.conv, c.bn)
            delattr(c, "bn")
    return m


@torch.no_grad()
def aattn_peaks(m: nn.Module, x: torch.Tensor) -> list[float]:
    """peakedness() of every AAttn inside the restated module m on input x, evaluated in fp64 after BN folding."""
    f = fuse_(copy.deepcopy(m).eval()).double()
    got, hooks = [], []
    for a in f.modules():
        if isinstance(a, AAttn):
            hooks.append(a.qkv.register_forward_hook(
                lambda mod, inp, out, a=a: got.append(peakedness(out.permute(0, 2, 3, 1), a.num_heads, a.area))))
    f(x.double())
    for h in hooks:
        h.remove()
    return got


@torch.no_grad()
def sharpen_(m: nn.Module, x: torch.Tensor, floor: float = 0.2) -> list[float]:
    """Make the attention of a restated module matter on input x: v rows of every qkv and every proj x 8 (the
    attention branch is not lost under the residual), q / k rows x 2 until every AAttn's peakedness is >= floor.
    Returns the final peakedness values."""
    attns = [a for a in m.modules() if isinstance(a, AAttn)]
    for a in attns:
        w = a.qkv.conv.weight.view(a.num_heads, 96, -1)
        w[:, 64:] *= 8.0
        a.proj.conv.weight *= 8.0
    for _ in range(24):
        peaks = aattn_peaks(m, x)
        if min(peaks) >= floor:
            return peaks
        for a, p in zip(attns, peaks):
            if p < floor:
                a.qkv.conv.weight.view(a.num_heads, 96, -1)[:, :64] *= 2.0
    raise AssertionError(f"could not reach peakedness {floor}: {peaks}")


@torch.no_grad()
def legs(fused: nn.Module, x: torch.Tensor):
    """(fp64, fp32, fp16) outputs of a BN-folded restated module by torch-CPU."""
    return (copy.deepcopy(fused).double()(x.double()), fused(x), copy.deepcopy(fused).half()(x.half()))
