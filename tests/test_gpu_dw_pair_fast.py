"""csrc/dw_pair.hip's padded-map kernel for the LSK depthwise pair (dw 5x5 -> dw 7x7 dilation 3, fp16) against the
tap-skipping dw_pair_kernel (YDBL_DW_PAIR_OLD=1), the two ydbl_dwconv2d_nhwc launches, and a numpy fp32 restatement,
bit for bit on both outputs.

The padded-map kernel keeps the padded taps as fma(0, w, acc) terms; the others skip them.  With finite weights the
two are the same number: acc starts at +0, and round-to-nearest never turns it into -0.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROUTE_TWO, ROUTE_OLD, ROUTE_FAST = 0, 1, 2

# (n, c, h, w), the kernel the library must choose by default
CASES = [
    ((3, 16, 1, 1), ROUTE_FAST),      # one pixel: every tap but the centre is padding
    ((1, 32, 7, 5), ROUTE_FAST),      # every tap row touches padding
    ((2, 256, 20, 20), ROUTE_FAST),   # the P5 map of the 640 networks
    ((3, 64, 16, 32), ROUTE_FAST),    # the 512-pixel limit, 77 440 B of LDS
    ((2, 48, 19, 3), ROUTE_FAST),     # three channel groups, a ragged last wave
    ((1, 32, 2, 256), ROUTE_OLD),     # 512 pixels whose padded maps (225 280 B) do not fit: the old kernel
]


def _convs(c, bias, seed):
    import torch.nn as nn

    g = torch.Generator().manual_seed(seed)
    c0 = nn.Conv2d(c, c, 5, padding=2, groups=c, bias=bias)
    c1 = nn.Conv2d(c, c, 7, padding=9, groups=c, dilation=3, bias=bias)
    with torch.no_grad():  # fp16-valued taps: every product with an fp16 x is exact in fp32
        c0.weight.copy_((torch.randn(c, 1, 5, 5, generator=g) * 0.3).half().float())
        c1.weight.copy_((torch.randn(c, 1, 7, 7, generator=g) * 0.3).half().float())
        if bias:
            c0.bias.copy_(torch.randn(c, generator=g) * 0.5)
            c1.bias.copy_(torch.randn(c, generator=g) * 0.5)
    return c0, c1


def _pair_plan(x, c0, c1, sliced):
    """One ydbl_dwconv2d_pair_nhwc launch on x; sliced: x, a1 and a2 are channel slices of wider buffers."""
    from ydbl.nn import modules as M
    from ydbl.runtime import Plan

    plan = Plan(torch.device(DEV), torch.float16)
    n, c, h, w = x.shape

    def view(off, extra):
        if not sliced:
            return plan.alloc(n, h, w, c)
        buf = plan.alloc(n, h, w, c + off + extra)
        buf.torch().fill_(-3.0)  # neighbours of the slice: must stay as they are
        return buf.cslice(off, c)

    xv, a1, a2 = view(8, 16), view(16, 8), view(24, 0)
    xv.torch().copy_(x.permute(0, 2, 3, 1).to(torch.float16))
    descs, keep = [], []
    for conv, src, dst in ((c0, xv, a1), (c1, a1, a2)):
        b = conv.bias.detach().float() if conv.bias is not None else None
        d, kk = M.dw_desc(plan, src, dst, conv.weight.detach().float(), b, 1, conv.padding[0], conv.dilation[0])
        descs.append(d)
        keep += kk
    plan.launch("ydbl_dwconv2d_pair_nhwc", descs[0], descs[1], what="dw_pair", keep=keep)
    return plan, xv, a1, a2


def _run_pair(x, c0, c1, old, monkeypatch, sliced=False):
    """-> (route the library reports, a1, a2 as [n, h, w, c] CPU tensors, the untouched-neighbour check)."""
    from ydbl import _lib

    if old:
        monkeypatch.setenv("YDBL_DW_PAIR_OLD", "1")
    else:
        monkeypatch.delenv("YDBL_DW_PAIR_OLD", raising=False)
    plan, xv, a1, a2 = _pair_plan(x, c0, c1, sliced)
    d0, d1 = plan.steps[-1].args[:2]
    route = _lib.lib.ydbl_dwconv2d_pair_route(d0, d1)  # read under the same switch as the launch below
    plan.run()
    torch.cuda.synchronize()
    monkeypatch.delenv("YDBL_DW_PAIR_OLD", raising=False)
    if sliced:
        for v in (xv, a1, a2):
            whole = torch.as_strided(v.base, (v.n * v.h * v.w, v.cs), (v.cs, 1), 0)
            lo = v.off
            assert bool((whole[:, :lo] == -3.0).all()) and bool((whole[:, lo + v.c:] == -3.0).all())
    return route, a1.torch().cpu().clone(), a2.torch().cpu().clone()


def _two_launches(x, c0, c1):
    from ydbl.nn import modules as M
    from ydbl.runtime import Plan

    plan = Plan(torch.device(DEV), torch.float16)
    n, c, h, w = x.shape
    xv = plan.alloc(n, h, w, c)
    xv.torch().copy_(x.permute(0, 2, 3, 1).to(torch.float16))
    b1 = M.emit_conv2d(plan, c0, xv, None)
    b2 = M.emit_conv2d(plan, c1, b1, None)
    assert [st.fn.__name__ for st in plan.steps] == ["ydbl_dwconv2d_nhwc"] * 2
    plan.run()
    torch.cuda.synchronize()
    return b1.torch().cpu().clone(), b2.torch().cpu().clone()


def _dw_restated(x, w, b, k, pad, dil):
    """x [n, c, h, w], w [c, k, k], b [c] or None; fp32 arrays, x and w of fp16 values -> fp16 [n, c, h, w]:
    acc = float32(acc + x * w) in (ky, kx) order over the zero-padded map (each product exact, so an FMA equals
    multiply-then-add), the bias added after the chain, one rounding to fp16."""
    n, c, h, wd = x.shape
    xp = np.zeros((n, c, h + 2 * pad, wd + 2 * pad), np.float32)
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    acc = np.zeros((n, c, h, wd), np.float32)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky * dil:ky * dil + h, kx * dil:kx * dil + wd]
            prod = (win * w[None, :, ky, kx, None, None]).astype(np.float32)
            acc = (acc + prod).astype(np.float32)
    if b is not None:
        acc = (acc + b[None, :, None, None].astype(np.float32)).astype(np.float32)
    return acc.astype(np.float16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int16)


def _nchw_bits(t):
    return _bits(t.permute(0, 3, 1, 2).numpy())


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape,route", CASES, ids=["x".join(map(str, s)) for s, _ in CASES])
def test_dw_pair_fast_bit_identical(shape, route, bias, monkeypatch):
    n, c, h, w = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, c, h, w, generator=g).half().float()
    c0, c1 = _convs(c, bias, seed=c + h)
    r_new, n1, n2 = _run_pair(x, c0, c1, False, monkeypatch)
    r_old, o1, o2 = _run_pair(x, c0, c1, True, monkeypatch)
    assert (r_new, r_old) == (route, ROUTE_OLD)
    t1, t2 = _two_launches(x, c0, c1)
    assert torch.equal(n1, o1) and torch.equal(n2, o2)
    assert torch.equal(n1, t1) and torch.equal(n2, t2)
    b0 = c0.bias.detach().numpy() if bias else None
    b1 = c1.bias.detach().numpy() if bias else None
    want1 = _dw_restated(x.numpy(), c0.weight.detach().numpy()[:, 0], b0, 5, 2, 1)
    want2 = _dw_restated(want1.astype(np.float32), c1.weight.detach().numpy()[:, 0], b1, 7, 9, 3)
    assert np.array_equal(_nchw_bits(n1), _bits(want1))
    assert np.array_equal(_nchw_bits(n2), _bits(want2))


def test_dw_pair_fast_channel_slices(monkeypatch):
    """x, a1 and a2 as channel slices of wider buffers (channel stride != c): same bits, neighbours untouched."""
    shape = (2, 48, 19, 3)
    g = torch.Generator().manual_seed(99)
    x = torch.randn(*shape, generator=g).half().float()
    c0, c1 = _convs(shape[1], True, seed=5)
    r_new, n1, n2 = _run_pair(x, c0, c1, False, monkeypatch, sliced=True)
    r_old, o1, o2 = _run_pair(x, c0, c1, True, monkeypatch, sliced=True)
    assert (r_new, r_old) == (ROUTE_FAST, ROUTE_OLD)
    t1, t2 = _two_launches(x, c0, c1)
    assert torch.equal(n1, o1) and torch.equal(n2, o2)
    assert torch.equal(n1, t1) and torch.equal(n2, t2)


def test_dw_pair_route_fallbacks():
    """fp32 takes the old kernel; 24 x 24 (576 pixels) the two launches."""
    from ydbl import _lib
    from ydbl.nn import modules as M
    from ydbl.runtime import Plan

    c0, c1 = _convs(32, True, seed=1)
    for dtype, hw, want in ((torch.float32, 20, ROUTE_OLD), (torch.float16, 24, ROUTE_TWO)):
        plan = Plan(torch.device(DEV), dtype)
        M.emit_dw_pair(plan, c0, c1, plan.alloc(1, hw, hw, 32))
        d0, d1 = plan.steps[-1].args[:2]
        assert _lib.lib.ydbl_dwconv2d_pair_route(d0, d1) == want
