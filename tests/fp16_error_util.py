"""fp16 error statistics against an fp64 reference (tests/test_gpu_fp16_error.py, tests/test_fp16_error_host.py).

The model the caps come from: a kernel computes the exact value of its operation on the operands it holds
(fp32 accumulation noise aside) and rounds once, to nearest even, for every fp16 it stores.  In units of the
reference's fp16 ulp the error of such a store is uniform on [-0.5, 0.5]:

    unit(r) = 2^(floor(log2(max(|r|, 2^-4))) - 10)   the fp16 ulp of r, floored at the ulp of 1/16
    e       = (got - ref) / unit(ref)
    max|e|  = 0.5        (one rounding)
    f1      = 0          share of elements with |e| > 1
    rmsc    = 1/sqrt(12) = 0.289, sqrt(mean(clip(e, -1, 1)^2))
    bias    = 0          mean(sign(ref) * clip(e, -1, 1)): < 0 is a store that rounds toward zero

The floor: SiLU outputs and residual sums near zero have arbitrarily small ulps while the fp32 accumulation
noise is absolute, so below 1/16 the error is measured in the ulp of 1/16.  A test must then show that most of
its elements lie above the floor (MIN_ABOVE_FLOOR), or the unit would hide everything.

Caps (never loosened to make a kernel pass):

    statistic                       model   fp32 emulation   cap
    max|e|, stages == 1             0.5     <= 0.56          <= 1  (f1 = 0)
    max|e|, fp16 intermediates      -       2.06             <= 4
    f1,     fp16 intermediates      -       0.11 %           <= 0.5 %
    rmsc                            0.289   0.27 - 0.285     <= 0.33
    |bias|                          0       <= 0.007         <= 0.05

`stages` counts the fp16 roundings between the operands and the output: 1 for one accumulation, the epilogue and
one store; > 1 for kernels that keep an intermediate in fp16 (the rare element whose intermediate rounds the
other way under another summation order moves the output by more than a unit).  The bias cap is more than 10
sigma of the mean of MIN_ELEMENTS uniform rounding errors (0.289 / sqrt(4096) = 0.0045).
"""

from __future__ import annotations

import torch

FLOOR = 2.0 ** -4
MIN_ELEMENTS = 4096
MIN_ABOVE_FLOOR = 0.75
CAP_MAX_SINGLE = 1.0
CAP_MAX_STAGED = 4.0
CAP_F1_STAGED = 0.005
CAP_RMSC = 0.33
CAP_BIAS = 0.05
F16_OVERFLOW = 65520.0  # the smallest magnitude that rounds (to nearest even) to inf in fp16


def h16(t: torch.Tensor) -> torch.Tensor:
    """t as fp16 holds it, in float64: the rounding every fp16 operand and stored intermediate goes through."""
    return t.to(torch.float16).to(torch.float64)


def unit(ref: torch.Tensor, floor: float = FLOOR) -> torch.Tensor:
    """The fp16 ulp of each reference value, floored at the ulp of `floor`."""
    a = ref.detach().to(torch.float64).abs().clamp_min(floor)
    _, ex = torch.frexp(a)  # a = m * 2^ex, m in [0.5, 1): floor(log2(a)) = ex - 1
    return torch.ldexp(torch.ones_like(a), ex - 11)


def error_stats(got: torch.Tensor, ref: torch.Tensor, fixed_unit: float | None = None) -> dict:
    """max|e|, f1, rmsc, bias of `got` (any float dtype) against the fp64 `ref`; n and the share of |ref| >= FLOOR."""
    got = got.detach().cpu().to(torch.float64).reshape(-1)
    ref = ref.detach().cpu().to(torch.float64).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    u = torch.full_like(ref, fixed_unit) if fixed_unit is not None else unit(ref)
    e = (got - ref) / u
    c = e.clamp(-1.0, 1.0)
    return dict(n=ref.numel(), above=(ref.abs() >= FLOOR).double().mean().item(),
                finite=bool(torch.isfinite(got).all()), max=e.abs().max().item(),
                f1=(e.abs() > 1.0).double().mean().item(), rmsc=c.square().mean().sqrt().item(),
                bias=(torch.sign(ref) * c).mean().item())


def fmt(st: dict) -> str:
    return (f"max|e| {st['max']:.3f}  f1 {100 * st['f1']:.3f} %  rmsc {st['rmsc']:.4f}  bias {st['bias']:+.4f}  "
            f"(n {st['n']}, |ref| >= 2^-4: {100 * st['above']:.1f} %)")


def violations(st: dict, stages: int) -> list[str]:
    """The caps `st` misses, as text; empty when it meets them all."""
    bad = []
    if not st["finite"]:
        bad.append("non-finite output")
    if stages <= 1:
        if not st["max"] <= CAP_MAX_SINGLE:
            bad.append(f"max|e| {st['max']:.3f} > {CAP_MAX_SINGLE} (single stage)")
    else:
        if not st["max"] <= CAP_MAX_STAGED:
            bad.append(f"max|e| {st['max']:.3f} > {CAP_MAX_STAGED} (fp16 intermediates)")
        if not st["f1"] <= CAP_F1_STAGED:
            bad.append(f"f1 {st['f1']:.5f} > {CAP_F1_STAGED}")
    if not st["rmsc"] <= CAP_RMSC:
        bad.append(f"rmsc {st['rmsc']:.4f} > {CAP_RMSC}")
    if not abs(st["bias"]) <= CAP_BIAS:
        bad.append(f"|bias| {abs(st['bias']):.4f} > {CAP_BIAS}")
    return bad


def assert_fp16_accurate(got, ref, stages: int, emu=None, name: str = "") -> dict:
    """Hold the fp16 output `got` to the caps against the fp64 reference `ref`.

    stages: fp16 roundings between operands and output (1: single-stage kernel).  emu: the plain torch fp32 CPU
    emulation of the same operation rounded to fp16; when given it must meet the caps itself, so that a failure
    is the kernel's and not the inputs'.  Prints the statistics (pytest shows them on failure) and returns them."""
    st = error_stats(got, ref)
    print(f"fp16-error {name or 'kernel'}: {fmt(st)}")
    assert st["n"] >= MIN_ELEMENTS, f"{name}: {st['n']} compared elements < {MIN_ELEMENTS}"
    assert st["above"] >= MIN_ABOVE_FLOOR, (
        f"{name}: only {100 * st['above']:.1f} % of the reference is >= 2^-4: the unit floor would hide errors")
    if emu is not None:
        se = error_stats(emu, ref)
        print(f"fp16-error {name or 'kernel'} (fp32 CPU emulation): {fmt(se)}")
        bad = violations(se, stages)
        assert not bad, f"{name}: the fp32 emulation itself misses the caps (inputs unfit): {bad}; {fmt(se)}"
    bad = violations(st, stages)
    assert not bad, f"{name}: {'; '.join(bad)}\n  {fmt(st)}"
    return st


def silu64(v: torch.Tensor) -> torch.Tensor:
    """x * sigmoid(x) in float64, finite for any finite x (exp(-x) may overflow to inf: x / inf = 0)."""
    return v * torch.sigmoid(v)

