"""ydbl_area_attn (csrc/attn.hip) and ydbl_channel_gate_add alone, through the C ABI.

Inputs: q, k ~ N(0, 1.7^2), v ~ N(0, 1).  The gain is a CONDITION of the test, asserted on the fp64 reference: the
mean row-maximum softmax probability must be >= 0.2.  With the modules' init weights the softmax is exactly uniform
(max p = 1/T), and a kernel that ignored q.k would pass.

Reference: fp64 torch on the inputs as the GPU receives them (fp16-rounded in half mode).  Bound (parity_util's
convention): 2 x the max deviation from fp64 of the torch-CPU leg of the same precision (fp32: fp32 matmul and softmax;
half: half q^T k, half softmax, half P v) + one unit of roundoff of max|y| (2^-23 / 2^-10).
Measured on an MI355X, GPU deviation / CPU-leg deviation for T = 4, 15, 100, 400 (area 1), 1600, 400 (area 4):
fp32 0.66, 1.03, 1.12, 1.02, 1.66, 1.45; half 0.67, 0.31, 0.19, 0.16, 0.08, 0.12 -- the factor 2 holds as it stands.
"""

import ctypes as C
import functools

import pytest
import torch

import a2c2f_util as U

pytestmark = pytest.mark.gpu

CASES = [(2, 2, 2, 1, 1), (1, 6, 10, 2, 4), (2, 20, 20, 2, 4), (1, 20, 20, 4, 1), (1, 80, 80, 2, 4), (3, 40, 40, 2, 4)]
GAIN = 1.7
SENTINEL = 777.0


@functools.lru_cache(maxsize=None)
def reference(case, half):
    """(qkv as the GPU receives it [n,h,w,3C], y fp64, bound); computed once per (case, dtype) and not modified."""
    n, h, w, heads, area = case
    g = torch.Generator().manual_seed(hash(case) % (1 << 31))
    qkv = torch.randn(n, h, w, heads, 96, generator=g)
    qkv[..., :64] *= GAIN
    qkv = qkv.reshape(n, h, w, heads * 96)
    if half:
        qkv = qkv.half()
    y64 = U.attn_ref(qkv, heads, area, torch.float64)
    peak = U.peakedness(qkv, heads, area)
    assert peak >= 0.2, f"softmax too flat for the test to see q.k: mean row max {peak:.3f}"
    leg = U.attn_ref(qkv, heads, area, torch.float16 if half else torch.float32)
    e = (leg.double() - y64).abs().max().item()
    return qkv, y64, U.leg_bound(leg, y64, half), e, peak


def view(t, c0, c):
    """TV over channels [c0, c0+c) of a contiguous NHWC device tensor."""
    from ydbl.runtime import TV

    n, h, w, cs = t.shape
    return TV(t.view(-1), c0, n, h, w, c, cs)


def launch(qkv, heads, area, y_view, v_view):
    from ydbl import _lib
    from ydbl.nn.modules import _null_view

    d = _lib.AreaAttnDesc(view(qkv, 0, qkv.shape[3]).struct(), y_view.struct(),
                          v_view.struct() if v_view is not None else _null_view(), heads, area, 32**-0.5)
    _lib.check(_lib.lib.ydbl_area_attn(d, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ydbl_area_attn")
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", ["plain", "y_slice", "v_null"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_h%d_a%d" % c)
def test_area_attn(case, half, mode):
    n, h, w, heads, area = case
    C_ = heads * 32
    qkv, y64, bound, e, peak = reference(case, half)
    dt = qkv.dtype
    dq = qkv.cuda()
    # y: its own buffer, or channels [16, 16 + C) of a wider one whose other channels must stay untouched
    wide, c0 = (C_ + 40, 16) if mode == "y_slice" else (C_, 0)
    ybuf = torch.full((n, h, w, wide), SENTINEL, dtype=dt, device="cuda")
    vbuf = torch.full((n, h, w, C_), SENTINEL, dtype=dt, device="cuda") if mode != "v_null" else None
    launch(dq, heads, area, view(ybuf, c0, C_), view(vbuf, 0, C_) if vbuf is not None else None)
    yb = ybuf.cpu()
    y = yb[..., c0:c0 + C_]
    outside = torch.cat([yb[..., :c0], yb[..., c0 + C_:]], -1)
    assert torch.equal(outside, torch.full_like(outside, SENTINEL)), "wrote outside the y slice"
    assert torch.isfinite(y).all()
    d = (y.double() - y64).abs().max().item()
    print(f"area_attn {case} {'half' if half else 'fp32'} {mode}: T={h * w // area} peak={peak:.3f} "
          f"cpu leg e={e:.3g} gpu d={d:.3g} bound={bound:.3g} ratio d/e={d / max(e, 1e-30):.2f}")
    assert d <= bound
    if vbuf is not None:  # bit-equal to the V channels of the input
        want = qkv.reshape(n, h, w, heads, 96)[..., 64:].reshape(n, h, w, C_)
        assert torch.equal(vbuf.cpu(), want)


def test_area_attn_rejects_bad_geometry():
    from ydbl import _lib

    qkv = torch.zeros(1, 3, 5, 96, device="cuda")
    y = torch.zeros(1, 3, 5, 32, device="cuda")
    with pytest.raises(_lib.YdblError, match="multiple of area"):
        launch(qkv, 1, 4, view(y, 0, 32), None)  # 15 tokens, 4 areas
    with pytest.raises(_lib.YdblError, match="3 \\* heads"):
        launch(qkv, 2, 1, view(y, 0, 32), None)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_channel_gate_add(half):
    """y = a + g[c] * b against the fp32 expression, to 1 ulp of the output format, at (2, 5, 7, 24)."""
    from ydbl import _lib

    g_ = torch.Generator().manual_seed(5)
    dt = torch.float16 if half else torch.float32
    a = torch.randn(2, 5, 7, 24, generator=g_).to(dt)
    b = torch.randn(2, 5, 7, 24, generator=g_).to(dt)
    gate = torch.randn(24, generator=g_)
    da, db, dg = a.cuda(), b.cuda(), gate.cuda()
    y = torch.empty_like(da)
    _lib.check(_lib.lib.ydbl_channel_gate_add(view(da, 0, 24).struct(), view(db, 0, 24).struct(), dg.data_ptr(),
                                               view(y, 0, 24).struct(),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "channel_gate_add")
    torch.cuda.synchronize()
    ref = a.float() + gate * b.float()
    _, ex = torch.frexp(ref.abs().clamp_min(2.0**-14))  # |ref| = m * 2^ex, m in [0.5, 1)
    ulp = torch.ldexp(torch.ones_like(ref), ex - 1 - (10 if half else 23))  # spacing of the output format at ref
    assert ((y.cpu().float() - ref).abs() <= ulp).all()
