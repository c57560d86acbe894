"""The fp16 error statistics (tests/fp16_error_util.py) on the CPU: the caps accept the honest fp32 emulation of
conv + bias + SiLU (+ residual) and of the two-stage Bottleneck, and reject every planted defect that today's
rtol = atol = 1e-2 lets through.  This is what makes tests/test_gpu_fp16_error.py a test: a kernel with one of
these defects would fail it.

Emulation = the operation in torch fp32 on fp16-rounded activations and weights, fp32 bias, one round-to-nearest
store.  Reference = the same in float64.  Defects, each the emulation with one rounding point moved:
  act16      the activation rounded to fp16 before the residual add
  pre16      the pre-activation (accumulator + bias) rounded to fp16
  bias16     the bias held in fp16
  part16     the running sum rounded to fp16 after every 64 input channels
  mid32      the Bottleneck intermediate left in fp32 (the unfused path stores it as fp16)
  trunc      the output store truncating instead of rounding to nearest
"""

import pytest
import torch
import torch.nn.functional as F

from fp16_error_util import CAP_BIAS, assert_fp16_accurate, error_stats, fmt, h16, silu64, unit, violations

# (cin, cout, k, n, h, w, residual)
CONV_SHAPES = [(8, 16, 3, 2, 13, 11, True), (64, 64, 3, 2, 13, 11, True), (512, 96, 1, 2, 13, 11, True)]
BNECK_C = [16, 64]


def _trunc16(v):
    """fp32 -> fp16 rounding toward zero."""
    h = v.half()
    over = h.float().abs() > v.abs()
    bits = h.view(torch.int16) - over.to(torch.int16)  # sign-magnitude: one code less is one step toward zero
    return bits.view(torch.float16)


def _conv_case(cin, cout, k, n, h, w, res):
    g = torch.Generator().manual_seed(cin * 1000 + cout + k)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g)
    r = torch.randn(n, cout, h, w, generator=g) if res else None
    return x, wt, b, r


def _conv_ref(x, wt, b, r, k):
    y = silu64(F.conv2d(h16(x), h16(wt), b.double(), 1, k // 2))
    return y + h16(r) if r is not None else y


def _conv_emu(x, wt, b, r, k, defect=None):
    xf, wf, bf = x.half().float(), wt.half().float(), b.clone()
    if defect == "bias16":
        bf = bf.half().float()
    if defect == "part16":
        acc = torch.zeros(())
        for c0 in range(0, xf.shape[1], 64):
            acc = (acc + F.conv2d(xf[:, c0:c0 + 64], wf[:, c0:c0 + 64], None, 1, k // 2)).half().float()
        pre = acc + bf[None, :, None, None]
    else:
        pre = F.conv2d(xf, wf, bf, 1, k // 2)
    if defect == "pre16":
        pre = pre.half().float()
    y = F.silu(pre)
    if defect == "act16":
        y = y.half().float()
    if r is not None:
        y = y + r.half().float()
    return _trunc16(y) if defect == "trunc" else y.half()


def _bneck_case(c):
    g = torch.Generator().manual_seed(c * 7)
    n, h, w, cm = 2, 16, 16, c // 2
    x = torch.randn(n, c, h, w, generator=g)
    w1 = torch.randn(cm, c, 3, 3, generator=g) / (9 * c) ** 0.5
    b1 = torch.randn(cm, generator=g) * 0.5
    w2 = torch.randn(c, cm, 3, 3, generator=g) / (9 * cm) ** 0.5
    b2 = torch.randn(c, generator=g) * 0.5
    return x, w1, b1, w2, b2


def _bneck_ref(x, w1, b1, w2, b2):
    mid = h16(silu64(F.conv2d(h16(x), h16(w1), b1.double(), 1, 1)))
    return silu64(F.conv2d(mid, h16(w2), b2.double(), 1, 1)) + h16(x)


def _bneck_emu(x, w1, b1, w2, b2, defect=None):
    f = lambda t: t.half().float()
    mid = F.silu(F.conv2d(f(x), f(w1), b1, 1, 1))
    if defect != "mid32":
        mid = f(mid)
    y = F.silu(F.conv2d(mid, f(w2), b2, 1, 1)) + f(x)
    return _trunc16(y) if defect == "trunc" else y.half()


def test_unit_is_the_fp16_ulp():
    r = torch.tensor([1.0, 1.999, 2.0, -3.0, 0.5, 2.0 ** -4, 2.0 ** -4 - 1e-9, 0.0, 1e-6, 300.0, -40000.0])
    want = [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 2.0 ** -11, 2.0 ** -14, 2.0 ** -14, 2.0 ** -14, 2.0 ** -14,
            2.0 ** -2, 2.0 ** 5]
    assert unit(r).tolist() == want
    # the unit of every normal fp16 value at or above the floor is the spacing to its neighbour
    v = torch.arange(0x2C00, 0x7BFF, dtype=torch.int16).view(torch.float16)
    nxt = torch.arange(0x2C01, 0x7C00, dtype=torch.int16).view(torch.float16)
    assert torch.equal(unit(v.double()), nxt.double() - v.double())


def test_stats_of_known_errors():
    ref = torch.full((8192,), 1.5, dtype=torch.float64)
    u = 2.0 ** -10
    got = ref.clone()
    got[::2] += 0.5 * u
    got[1::2] -= 0.5 * u
    st = error_stats(got, ref)
    assert st["max"] == 0.5 and st["f1"] == 0.0 and abs(st["rmsc"] - 0.5) < 1e-12 and st["bias"] == 0.0
    got = ref - 0.25 * u  # toward zero
    st = error_stats(got, ref)
    assert st["bias"] == -0.25 and violations(st, 1) == [f"|bias| 0.2500 > {CAP_BIAS}"]
    st = error_stats(-got, -ref)  # sign(ref) makes "toward zero" negative on either side
    assert st["bias"] == -0.25
    got = ref.clone()
    got[:82] += 3 * u  # 1 % of the elements 3 units off
    st = error_stats(got, ref)
    assert st["max"] == 3.0 and abs(st["f1"] - 82 / 8192) < 1e-12
    assert violations(st, 1) and violations(st, 2)  # over max|e| <= 1, and over f1 <= 0.5 %
    got[0] = float("nan")
    assert "non-finite output" in violations(error_stats(got, ref), 2)


def test_inputs_are_checked():
    ref = torch.randn(1000, dtype=torch.float64) + 3
    with pytest.raises(AssertionError, match="compared elements"):
        assert_fp16_accurate(ref.half(), ref, 1)
    ref = torch.randn(8192, dtype=torch.float64) * 0.03  # mostly under the floor
    with pytest.raises(AssertionError, match="unit floor"):
        assert_fp16_accurate(ref.half(), ref, 1)
    ref = torch.randn(8192, dtype=torch.float64) + 3
    with pytest.raises(AssertionError, match="emulation itself"):
        assert_fp16_accurate(ref.half(), ref, 1, emu=(ref * 1.01).half())


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: f"{s[0]}to{s[1]}k{s[2]}")
def test_conv_emulation_meets_the_caps(shape):
    cin, cout, k, n, h, w, res = shape
    x, wt, b, r = _conv_case(*shape)
    ref = _conv_ref(x, wt, b, r, k)
    st = assert_fp16_accurate(_conv_emu(x, wt, b, r, k), ref, 1, name=f"emulation {cin}->{cout} k{k}")
    assert st["max"] <= 0.6  # one rounding + the fp32 accumulation noise


@pytest.mark.parametrize("defect", ["act16", "pre16", "bias16", "part16", "trunc"])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: f"{s[0]}to{s[1]}k{s[2]}")
def test_conv_defect_is_rejected(shape, defect):
    cin, cout, k, n, h, w, res = shape
    x, wt, b, r = _conv_case(*shape)
    ref = _conv_ref(x, wt, b, r, k)
    got = _conv_emu(x, wt, b, r, k, defect)
    st = error_stats(got, ref)
    print(defect, fmt(st))
    bad = violations(st, 1)
    assert bad, f"{defect} passes the caps: {fmt(st)}"
    if defect == "trunc":
        assert st["bias"] < -0.2 and any("bias" in m for m in bad)
    # and today's tolerance cannot see it
    torch.testing.assert_close(got.double(), ref, rtol=1e-2, atol=1e-2)
    with pytest.raises(AssertionError):
        assert_fp16_accurate(got, ref, 1, emu=_conv_emu(x, wt, b, r, k))


@pytest.mark.parametrize("c", BNECK_C)
def test_bottleneck_emulation_meets_the_caps(c):
    args = _bneck_case(c)
    st = assert_fp16_accurate(_bneck_emu(*args), _bneck_ref(*args), 2, name=f"emulation Bottleneck c{c}")
    assert st["max"] <= 4.0


@pytest.mark.parametrize("defect", ["mid32", "trunc"])
@pytest.mark.parametrize("c", BNECK_C)
def test_bottleneck_defect_is_rejected(c, defect):
    args = _bneck_case(c)
    ref = _bneck_ref(*args)
    got = _bneck_emu(*args, defect=defect)
    st = error_stats(got, ref)
    print(defect, fmt(st))
    assert violations(st, 2), f"{defect} passes the caps: {fmt(st)}"
    torch.testing.assert_close(got.double(), ref, rtol=1e-2, atol=1e-2)
