"""The oracle's side of the embed() tests (test infrastructure; imports oracle/).

oracle.model.DetectionModel.forward drops the layer outputs no later layer reads, so the embedding is restated here
as the reference computes it (U/nn/tasks.py:158-171): the same layer loop, each named layer's output pooled by
adaptive_avg_pool2d(x, (1, 1)) and the pooled vectors concatenated in layer order, stopping at max(embed).
"""

from __future__ import annotations

import copy

import torch
import torch.nn.functional as F


@torch.inference_mode()
def oracle_embed(o, x, embed):
    """[B, sum C_i] embedding of the (fused) oracle model `o` on x, in o's / x's dtype."""
    embed = set(embed)
    y, out = [], []
    for m in o.model:
        if m.f != -1:
            x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
        x = m(x)
        y.append(x if m.i in o.save else None)
        if m.i in embed:
            out.append(F.adaptive_avg_pool2d(x, (1, 1)).squeeze(-1).squeeze(-1))
        if m.i == max(embed):
            return torch.cat(out, 1)
    raise ValueError(f"embed {sorted(embed)} names no layer of the model")


def oracle_embed_legs(o, x, embed, legs=("fp64", "fp32", "fp16")):
    """{leg: [B, D] float64} of the oracle in each precision (parity_util.oracle_legs' three legs)."""
    out = {}
    for leg in legs:
        dt = {"fp64": torch.float64, "fp32": torch.float32, "fp16": torch.float16}[leg]
        m = o if leg == "fp32" else copy.deepcopy(o).to(dt)
        out[leg] = oracle_embed(m, x.to(dt), embed).double()
    return out


def pool_bound(v: torch.Tensor, fp16: bool) -> torch.Tensor:
    """Per (image, channel) error bound of a global average pool of the NHWC view v [n, h, w, c] against its fp64
    mean, derived: an fp32 sum of h*w terms in any order is off by at most (h*w - 1) * 2^-24 * sum|x| and the one
    division adds 2^-24 * |mean|, together at most h*w * 2^-24 * mean|x|; fp16 inputs convert to fp32 exactly and
    the one rounding of the result adds half an fp16 ulp of it (the ulp of the exact mean's binade; 2^-25 below the
    normal range)."""
    hw = v.shape[1] * v.shape[2]
    d = v.double()
    b = hw * 2.0 ** -24 * d.abs().mean((1, 2))
    if fp16:
        e = torch.frexp(d.mean((1, 2)).abs().clamp_min(2.0 ** -14)).exponent - 1  # |mean| in [2^e, 2^(e+1))
        b = b + 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 10).double())
    return b
