"""ydbl_maxpool5_cascade and ydbl_psa_attn on the MI355X.

The pool cascade is exact: torch.equal against three chained F.max_pool2d(., 5, 1, 2), fp32 and fp16, on maps smaller
than the 13-window, on one pixel, on strictly negative inputs (zero padding would fail) and into slices of a wider
buffer whose other channels must stay untouched.

The attention core is judged against the restated Attention core (tests/yolo11_util.py) evaluated by torch-CPU in
fp64; bound = a2c2f_util.leg_bound: 2 x the same-precision torch-CPU leg's max deviation from fp64 + one roundoff of
max|y|.  The inputs are scaled so that the softmax is peaked (floor 0.2 asserted): with a uniform softmax a wrong
kernel would pass."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import yolo11_util as U

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16]
IDS = ["fp32", "half"]


def _plan(dtype):
    from ydbl.runtime import Plan

    return Plan(torch.device("cuda"), dtype)


def _cascade(x):
    ys = [x]
    for _ in range(3):
        ys.append(F.max_pool2d(ys[-1], 5, 1, 2))
    return ys[1:]


# ----------------------------------------------------------------------------------------------- max-pool cascade
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape,negative", [((2, 20, 20, 128), False), ((1, 5, 7, 16), True), ((1, 1, 1, 8), True),
                                            ((3, 9, 33, 40), False)],
                         ids=["p5_640", "clipped_5x7", "one_pixel", "two_tiles_wide"])
def test_maxpool5_cascade_dense(shape, negative, dtype):
    from ydbl import _lib

    n, h, w, c = shape
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(h * w + c))
    if negative:
        x = -x.abs() - 0.25  # strictly negative: padding with 0 instead of -inf would win every border window
    x = x.to(dtype)
    plan = _plan(dtype)
    xv = plan.alloc(n, h, w, c)
    xv.torch().copy_(x.permute(0, 2, 3, 1))
    ys = [plan.alloc(n, h, w, c) for _ in range(3)]
    for y in ys:
        y.torch().fill_(7.0)
    d = _lib.MaxPool5Desc(xv.struct(), *[y.struct() for y in ys], 5)
    plan.launch("ydbl_maxpool5_cascade", d, what="pool", keep=[d])
    plan.run()
    torch.cuda.synchronize()
    for got, want in zip(ys, _cascade(x.float().cpu())):
        assert torch.equal(got.nchw().float().cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_maxpool5_cascade_into_concat_slices(dtype):
    """[2,13,40,24] written SPPF's way: x is slice 0 of a wider buffer, the outputs the next three slices; the
    channels around them (pre-filled with 5.0) stay as they were."""
    from ydbl import _lib

    n, h, w, c = 2, 13, 40, 24
    x = (-torch.rand(n, c, h, w, generator=torch.Generator().manual_seed(40)) - 0.5).to(dtype)
    plan = _plan(dtype)
    buf = plan.alloc(n, h, w, 8 + 4 * c + 16)
    buf.torch().fill_(5.0)
    sl = [buf.cslice(8 + i * c, c) for i in range(4)]
    sl[0].torch().copy_(x.permute(0, 2, 3, 1))
    d = _lib.MaxPool5Desc(*[s.struct() for s in sl], 5)
    plan.launch("ydbl_maxpool5_cascade", d, what="pool", keep=[d])
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(sl[0].nchw().cpu(), x)
    for got, want in zip(sl[1:], _cascade(x.float().cpu())):
        assert torch.equal(got.nchw().float().cpu(), want)
    rest = torch.cat([buf.torch()[..., :8], buf.torch()[..., 8 + 4 * c:]], -1).cpu()
    assert torch.equal(rest, torch.full_like(rest, 5.0))


# ----------------------------------------------------------------------------------------------- attention core
def _qkv(n, h, w, heads, floor=0.2):
    """A random NHWC qkv [n,h,w,heads*128] with q and k scaled until the fp64 peakedness is >= floor (one token: the
    softmax is 1), v of order 1."""
    g = torch.Generator().manual_seed(1000 * n + 10 * h * w + heads)
    t = torch.randn(n, h, w, heads, 128, generator=g)
    for _ in range(24):
        if U.peakedness(t.reshape(n, h, w, heads * 128), heads) >= floor:
            break
        t[..., :64] *= 1.5
    return t.reshape(n, h, w, heads * 128)


@pytest.fixture(scope="module")
def attn_case():
    """(n, h, w, heads) -> (qkv, peak, {dtype: (y leg, v)}, y64); computed once."""
    cache = {}

    def get(key):
        if key not in cache:
            n, h, w, heads = key
            qkv = _qkv(n, h, w, heads)
            y64, _ = U.psa_ref(qkv.half().float(), heads, torch.float64)  # the fp16-representable input, both dtypes
            legs = {dt: U.psa_ref(qkv.half().float(), heads, dt) for dt in DTYPES}
            cache[key] = (qkv.half().float(), U.peakedness(qkv.half().float(), heads), legs, y64)
        return cache[key]

    return get


def _run_attn(qkv, heads, dtype, with_v=True):
    from ydbl import _lib
    from ydbl.nn.modules import _null_view

    n, h, w, _ = qkv.shape
    plan = _plan(dtype)
    qv = plan.alloc(n, h, w, heads * 128)
    qv.torch().copy_(qkv.to(dtype))
    y, v = plan.alloc(n, h, w, heads * 64), plan.alloc(n, h, w, heads * 64)
    y.torch().fill_(float("nan"))
    v.torch().fill_(3.0)
    d = _lib.PsaAttnDesc(qv.struct(), y.struct(), v.struct() if with_v else _null_view(), heads, 32, 64, 32**-0.5)
    plan.launch("ydbl_psa_attn", d, what="attn", keep=[d])
    plan.run()
    torch.cuda.synchronize()
    first = y.torch().cpu().clone()
    y.torch().fill_(float("nan"))
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(first, y.torch().cpu())  # bit-identical on a second run
    return first, v.torch().cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("heads", [2, 6])
@pytest.mark.parametrize("n,h,w", [(2, 20, 20), (2, 7, 9), (1, 4, 4), (3, 1, 1)],
                         ids=["400tok", "63tok", "16tok", "1tok"])
def test_psa_attn(attn_case, n, h, w, heads, dtype):
    qkv, peak, legs, y64 = attn_case((n, h, w, heads))
    assert peak >= 0.2, peak
    half = dtype == torch.float16
    leg, vref = legs[dtype]
    bound = U.leg_bound(leg, y64, half)
    got, v = _run_attn(qkv, heads, dtype, with_v=True)
    assert torch.isfinite(got).all()
    d = (got.double() - y64).abs().max().item()
    e = (leg.double() - y64).abs().max().item()
    print(f"psa_attn N={h * w} heads={heads} {'half' if half else 'fp32'}: peak {peak:.3f} max|y|={y64.abs().max():.3g}"
          f" cpu leg e={e:.3g} gpu d={d:.3g} bound={bound:.3g}")
    assert torch.equal(v, vref)  # the re-laid V: bit copies
    assert d <= bound


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_psa_attn_null_v(attn_case, dtype):
    """A null v view skips the V output: y is the same bits, the buffer that would have been v is untouched."""
    qkv, _, _, _ = attn_case((2, 7, 9, 2))
    with_v, _ = _run_attn(qkv, 2, dtype, with_v=True)
    without, v = _run_attn(qkv, 2, dtype, with_v=False)
    assert torch.equal(with_v, without)
    assert torch.equal(v, torch.full_like(v, 3.0))
