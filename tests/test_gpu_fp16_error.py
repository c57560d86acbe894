"""The fp16 conv kernels held to rounding accuracy against float64 (statistics and caps: tests/fp16_error_util.py;
that the caps reject a subtly wrong kernel: tests/test_fp16_error_host.py).

Every reference runs the operation in float64 on the operands as the kernel holds them and rounds to fp16 wherever
the kernel stores or stages an fp16.  The rounding points, with the kernel line that makes each true:

dense convs (ydbl_conv2d_nhwc: block implicit GEMM, pointwise, wave-split-K, workspace split-K, halo, spatial tile,
VGPR-weight kernel -- one epilogue, csrc/conv_common.hpp conv_epilogue_as):
  x, residual  fp16 (the activation buffers)
  w            fp16 (modules.emit_dense: wk32.to(plan.dtype))
  bias         fp32 (emit_dense: plan.const(b.float()); epilogue "acc * dqv + bv")
  accumulator  fp32 MFMA; split-K partial tiles fp32 (conv.hip splitk_epilogue_kernel sums f32x4 from p.ws)
  act, res     fp32 ("act_as<T, A>(acc + bv)", then "add_rn(rv, v)" / "rv * v")
  y            one rounding (store_f -> common.hpp f16_rne)
  y2           pad_mix(a2, round_to<T>(v), b2, r2): the FullPAD second output reads y as stored, so its reference
               is a2 * (the kernel's own y) + b2 * r2 with one rounding
depthwise (csrc/misc.hip dwconv_kernel / dwconv_lds_kernel / dw_pair_kernel):
  w fp32 UNROUNDED (modules.dw_desc: plan.const(w.float())), bias fp32, fp32 FMAs, one rounding; the pair's second
  conv reads the first output as stored ("t[q] = (T)round_to<T>(o[q])"): reference from the kernel's own y0
fused DSConv / Detect DWConv -> Conv1x1 (csrc/dsconv_kernel.hpp, csrc/dsc_lean.hpp):
  dw taps ROUNDED to fp16 ("taps rounded to the activation dtype": s_w = float(T(wr))), dw bias fp32, dw
  activation fp32, depthwise value rounded to fp16 into the MFMA B tile (store4 -> to_h4_rne; dsc_lean.hpp
  "to_h4_rne(a[c])"), pw w fp16 (emit_dsconv: .to(plan.dtype)), pw bias fp32, one rounding of y; the class tail
  reads y as stored ("round_to<T>(v[q])", conv_common.hpp conv_tail_1x1*) with fp32 UNROUNDED tail weights and bias
  (emit_dsconv: plan.const(tail[0].float())): reference from the kernel's own y
Bottleneck / Detect box (csrc/bneck_kernel.hpp): w1, w2, w3 fp16 (pack: "(_Float16)w1[...]"; bneck.hip "(_Float16)w3"),
  biases fp32, cv1 output rounded to fp16 in LDS (epi1: "o[q] = f16_rne(inside ? sv : 0.f)"), pw = 1: cv2 output
  rounded to fp16 in LDS (epi2: "o[q] = f16_rne(v[q])"), one rounding of y
stem (csrc/stem.hip): image rounded to fp16 ("pack": round_to<T>(c * scale)), w ROUNDED to fp16 ("afrag = T(wv)"),
  bias fp32, one rounding
stem2 (csrc/stem2.hip): image fp16 ("f16_rne(v * scale)"), w0, w1 fp16 (pack: "(_Float16)wv"), the FIRST conv's
  bias fp16: it enters the MFMA as the centre tap's weight on a constant-1 record slot (stem2_pack: "c < 3 ? w0[...]
  : tap == 4 ? b0[co] : 0.f" -> "(_Float16)wv"), a documented choice (include/ydbl.h, ydbl_stem2_desc: "The first
  conv's bias enters the MFMA as an fp16 weight ... the second conv's is added in fp32"); layer-0 map rounded to
  fp16 in LDS ("hv[q] = f16_rne(silu_fast(acc[q]))"), second bias fp32, one rounding of y

Not here: the fp8 conv (test_gpu_ops.py::test_conv_fp8 keeps it).  Against its CPU emulation carried out in float64
(x * qs rounded to e4m3, e4m3 weights, "acc * dq + bias" with the calibration's bias correction, one fp16 rounding)
it misses max|e| <= 1 on 0.03-0.09 % of the elements (96->40 3x3: max|e| 1.15, f1 0.026 %, rmsc 0.292; 128->128 1x1
add: 3.33, 0.090 %, 0.293; 512->96 1x1: 1.39, 0.036 %, 0.291).  Those elements are not an activation with another
e4m3 code -- that would move every output channel of a pixel, and they are spread one to five channels to a pixel
(593 elements in 506 pixels of 128 channels) -- but results near zero whose conv term is about 2^-14 of its own
magnitude off: more than fp32 accumulation gives, so the sums of the fp8 matrix instruction are the suspect.
DESIGN.md section 2 has the figures.

stages = 1 where the reference takes every fp16 intermediate from the kernel's own output (no second rounding
of ours in between), 2 or 3 where an intermediate lives only in LDS.
"""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from fp16_error_util import F16_OVERFLOW, assert_fp16_accurate, error_stats, fmt, silu64, unit

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32


def _plan():
    from ydbl.runtime import Plan

    return Plan(torch.device(DEV), torch.float16)


def _tv(plan, x, cs_extra=8, c_off=8):
    """Upload an NCHW CPU tensor into a channel slice of a wider NHWC device buffer."""
    from ydbl.runtime import round_up

    n, c, h, w = x.shape
    cs = round_up(c + c_off + cs_extra, 8)
    buf = plan.alloc(n, h, w, cs)
    buf.torch().zero_()
    v = buf.cslice(c_off, c) if (c_off or cs != c) else buf
    v.torch().copy_(x.permute(0, 2, 3, 1).to(torch.float16))
    return v


def _out(plan, n, h, w, c):
    """An output view that is a channel slice of a wider buffer."""
    return plan.alloc(n, h, w, c + 16).cslice(8, c)


def _run(plan):
    plan.run()
    torch.cuda.synchronize()


def _host(v):
    return v.nchw().cpu().contiguous()


def _rd(t, dt):
    """t as fp16 holds it, in dtype dt."""
    return t.to(torch.float16).to(dt)


def _act(v, act):
    if act == "none":
        return v
    return silu64(v) if v.dtype == F64 else F.silu(v)


def _act_code(act):
    from ydbl import _lib

    return _lib.ACT_SILU if act == "silu" else _lib.ACT_NONE


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------- value ranges
def _vary(variant, b, act, scale_in, scale_w):
    """Part 3's value ranges on one conv stage: returns (bias, act, input scale, weight scale).  b: the unit-scale
    bias N(0, 1).  large: inputs x 2^6 and the bias at 640 + 64 N(0, 1), ten sigma of the conv's own spread: every
    result is large (fp32 accumulation noise and a flipped fp16 intermediate are both 2^6 larger in absolute terms
    here, so a result that cancels to near zero would be measured against a unit that is 2^6 too small; SiLU's
    negative side has its own case, tails).  overflow: the same without activation, two channels' bias at +-65450
    so their results (sigma = 64) straddle 65520.
    tails: channel thirds with the pre-activation near +30, -30 and -200.  small: inputs and weights x 2^-9, results
    ~ 2^-18 N(0, 1): fp16 subnormals."""
    c = b.numel()
    if variant == "large":
        return b * 64 + 640, "silu", 64.0, 1.0
    if variant == "overflow":
        b = b * 64 + 640
        b[0], b[1] = 65450.0, -65450.0
        return b, "none", 64.0, 1.0
    if variant == "tails":
        t = torch.full((c,), -200.0)
        t[: c // 3] = 30.0
        t[c // 3: 2 * (c // 3)] = -30.0
        return t + 0.5 * b, "silu", 1.0, 1.0
    if variant == "small":
        return b * 2.0 ** -18, "none", 2.0 ** -9, 2.0 ** -9
    assert variant is None
    return b, act, scale_in, scale_w


def _check(name, got, ref, stages, emu, variant):
    """The assertions of one case.  got / emu: fp16 [n, c, h, w]; ref: float64."""
    got = got.to(F64)
    assert not torch.isnan(got).any(), f"{name}: NaN in the output"
    if variant in (None, "large"):
        return assert_fp16_accurate(got, ref, stages, emu=emu, name=name)
    if variant == "overflow":
        want_inf = torch.isinf(ref.to(torch.float16))
        near = (ref.abs() - F16_OVERFLOW).abs() <= unit(ref)  # within one unit of the overflow point: either side
        share = near.double().mean().item()
        print(f"fp16-error {name}: {int(want_inf.sum())} infinite, {100 * share:.2f} % within a unit of 65520")
        assert want_inf.any() and (~want_inf & (ref.abs() > 65000)).any(), "the reference does not straddle 65520"
        assert share <= 0.02, share
        keep = ~near
        assert torch.equal(torch.isinf(got)[keep], want_inf[keep]), (
            int((torch.isinf(got) != want_inf)[keep].sum()), "elements overflow on the wrong side")
        assert torch.equal(torch.sign(got[want_inf & keep]), torch.sign(ref[want_inf & keep]))
        fin = keep & ~want_inf
        return assert_fp16_accurate(got[fin], ref[fin], stages, emu=emu[fin] if emu is not None else None, name=name)
    if variant == "tails":
        c = ref.shape[1]
        a, b = c // 3, 2 * (c // 3)
        assert torch.isfinite(got).all(), f"{name}: inf in the output"
        assert (ref[:, :a] > 20).all() and (ref[:, a:].to(torch.float16) == 0).all(), "the reference misses its tails"
        zero = got[:, a:] == 0
        assert zero.all(), f"{name}: {int((~zero).sum())} nonzero outputs at pre-activation -30 / -200"
        return assert_fp16_accurate(got[:, :a], ref[:, :a], stages, emu=emu[:, :a] if emu is not None else None,
                                    name=name)
    assert variant == "small"
    sub = ref.abs() < 2.0 ** -14
    nz = sub & (ref.abs() >= 2.0 ** -25)
    assert ref.numel() >= 4096 and sub.all() and nz.double().mean().item() >= 0.5, (
        sub.double().mean().item(), nz.double().mean().item())
    st = error_stats(got, ref, fixed_unit=2.0 ** -24)
    print(f"fp16-error {name} (unit 2^-24): {fmt(st)}")
    assert st["finite"] and st["max"] <= 1.0, f"{name}: subnormal results off by {st['max']:.2f} x 2^-24"
    assert (got[nz] != 0).double().mean().item() > 0.99, f"{name}: subnormal results flushed to zero"
    return st


# ------------------------------------------------------------------------------------------- dense convs
# name: (cin, cout, k, stride, act, residual, n, h, w, environment, options)
# environment: a value of None unsets the switch
# options: seeds (pool that many draws: the shape alone has < 4096 outputs), ws (the launch must get a split-K
# workspace), second (the fused FullPAD second output), route (the kernel family ydbl_conv_route must report under the
# case's environment: the switch reaches the kernel the case is named for; with the halo kernel's images per workgroup)
DENSE = {
    # block implicit GEMM and pointwise, the test_conv_dense shapes at 2 x 13 x 11
    "igemm-64-64-k3-add": (64, 64, 3, 1, "silu", "add", 2, 13, 11, {}, {}),
    "igemm-72-22-k3-mul": (72, 22, 3, 1, "none", "mul", 2, 13, 11, {}, {}),
    "igemm-16-32-k3-s2": (16, 32, 3, 2, "silu", None, 2, 13, 11, {}, {"seeds": 2}),
    "pw-24-80": (24, 80, 1, 1, "none", None, 2, 13, 11, {}, {}),
    "pw-32-48-mul": (32, 48, 1, 1, "silu", "mul", 2, 13, 11, {}, {}),
    "pw-32-48-second": (32, 48, 1, 1, "silu", "add", 2, 13, 11, {}, {"second": True}),
    # wave-split-K (K >= 512 on a small map)
    "wsk-512-96-k1-add": (512, 96, 1, 1, "silu", "add", 2, 13, 11, {}, {}),
    "wsk-256-32-k3": (256, 32, 3, 1, "silu", None, 2, 13, 11, {}, {}),
    # workspace split-K: wave-split-K over k-block steps, and the halo kernel over input-channel chunks
    "splitk-512-64-k3": (512, 64, 3, 1, "silu", None, 2, 20, 20, {}, {"ws": True}),
    "halo-split-384-128": (384, 128, 3, 1, "silu", None, 2, 40, 40, {}, {"ws": True}),
    # the other 3x3 routes, each at the smallest case of its test in test_gpu_ops.py that has >= 4096 outputs
    "halo-s1": (64, 32, 3, 1, "silu", None, 2, 161, 163, {"YDBL_HALO_NB": "1"}, {"route": ("HALO", 1)}),
    "halo-s2": (64, 64, 3, 2, "silu", None, 8, 320, 320, {}, {}),
    "halo-small-map": (64, 128, 3, 1, "silu", None, 3, 37, 41, {"YDBL_HALO_SMALL": "1"}, {"route": ("HALO", 2)}),
    "halo-nblock": (64, 96, 3, 1, "silu", None, 17, 37, 45, {"YDBL_HALO_NB": None, "YDBL_SPLITK": "0"}, {"route": ("HALO", 2)}),
    "tile-8-8": (8, 8, 3, 1, "silu", None, 2, 70, 66, {}, {}),
    "tile-16-32-s2-add": (16, 32, 3, 2, "silu", "add", 2, 131, 129, {}, {}),
    "vw-128-64-add": (128, 64, 3, 1, "silu", "add", 3, 21, 19, {"YDBL_VW": "1"}, {"route": ("VW", None)}),
}
# one shape per dense family for the value ranges (no residual there: the conv's own result is what is measured)
DENSE_RANGE = ["igemm-64-64-k3-add", "pw-24-80", "wsk-512-96-k1-add", "splitk-512-64-k3", "tile-16-32-s2-add"]


def _dense_draw(case, seed, variant):
    cin, cout, k, s, act, res, n, h, w, _, _ = case
    g = _gen(seed)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g)
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    r = None
    if res and variant in (None, "large"):
        r = torch.randn(n, cout, ho, wo, generator=g)
        if res == "mul":
            r = r + 1.5 * torch.sign(r)  # |r| >= 1.5: the product stays off the unit floor where the conv does
    b, act, sx, sw = _vary(variant, b, act, 1.0, 1.0)
    if variant == "large" and r is not None:
        r = r * 64
    r2 = torch.randn(n, cout, ho, wo, generator=g)
    return dict(x=x * sx, w=wt * sw, b=b, r=r, r2=r2, act=act, res=res if r is not None else None, k=k, s=s)


def _dense_math(d, dt):
    y = _act(F.conv2d(_rd(d["x"], dt), _rd(d["w"], dt), d["b"].to(dt), d["s"], d["k"] // 2), d["act"])
    if d["res"] == "add":
        y = _rd(d["r"], dt) + y
    elif d["res"] == "mul":
        y = _rd(d["r"], dt) * y
    return y


def _dense_gpu(d, opts):
    from ydbl import _lib
    from ydbl.nn.modules import emit_dense

    plan = _plan()
    xv = _tv(plan, d["x"])
    n, co = d["x"].shape[0], d["w"].shape[0]
    k, s = d["k"], d["s"]
    ho, wo = (xv.h + 2 * (k // 2) - k) // s + 1, (xv.w + 2 * (k // 2) - k) // s + 1
    yv = _out(plan, n, ho, wo, co)
    rv = _tv(plan, d["r"], 0, 0) if d["res"] else None
    mode = {None: _lib.RES_NONE, "add": _lib.RES_ADD, "mul": _lib.RES_MUL}[d["res"]]
    emit_dense(plan, xv, yv, d["w"], d["b"], s, k // 2, 1, _act_code(d["act"]), rv, mode)
    desc = plan.steps[-1].args[0]
    if opts.get("ws"):
        assert desc.workspace and desc.workspace_bytes == _lib.lib.ydbl_conv_workspace(desc) > 0
    if opts.get("route") or opts.get("ws"):
        route = _lib.ConvRouteInfo()
        _lib.check(_lib.lib.ydbl_conv_route(desc, route), "ydbl_conv_route")
        if opts.get("ws"):
            assert route.ksplit > 1, "the launch does not split"
        else:
            family, nb = opts["route"]
            assert route.family == getattr(_lib, "CONV_" + family) and nb in (None, route.v[1]), (
                route.family, list(route.v))
    y2 = None
    if opts.get("second"):
        y2 = _out(plan, n, ho, wo, co)
        assert plan.fuse_second_output(plan.writer_of(yv), y2, _tv(plan, d["r2"], 0, 0), 0.5, 1.0) is not None
    _run(plan)
    return _host(yv), (_host(y2) if y2 is not None else None)


def _dense_case(name, variant, monkeypatch):
    case = DENSE[name]
    env, opts = case[9], case[10]
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    gots, refs, emus, seconds = [], [], [], []
    for i in range(opts.get("seeds", 1)):
        d = _dense_draw(case, 1000 * case[0] + case[1] + case[2] + 7919 * i, variant)
        got, got2 = _dense_gpu(d, opts)
        gots.append(got)
        refs.append(_dense_math(d, F64))
        emus.append(_dense_math(d, F32).half())
        if got2 is not None:  # y2 = 0.5 * y + r2 on the y the kernel stored
            emu2 = (0.5 * got.float() + _rd(d["r2"], F32)).half()
            seconds.append((got2, 0.5 * got.to(F64) + _rd(d["r2"], F64), emu2))
    tag = f"{name}{'/' + variant if variant else ''}"
    _check(tag, torch.cat(gots), torch.cat(refs), 1, torch.cat(emus), variant)
    for got2, ref2, emu2 in seconds:
        _check(tag + " (second output)", got2, ref2, 1, emu2, None)


@pytest.mark.parametrize("name", list(DENSE))
def test_dense_conv(name, monkeypatch):
    _dense_case(name, None, monkeypatch)


@pytest.mark.parametrize("variant", ["large", "overflow", "tails", "small"])
@pytest.mark.parametrize("name", DENSE_RANGE)
def test_dense_conv_value_range(name, variant, monkeypatch):
    _dense_case(name, variant, monkeypatch)


# ------------------------------------------------------------------------------------------- depthwise
# (c, k, stride, dilation, bias, residual): test_dwconv's cases (the one-thread-per-vector kernel), and 64
# channels for every geometry the LDS-tiled kernel is built for (misc.hip launch_dw_lds)
DW = [(16, 3, 1, 1, False, False), (32, 3, 2, 1, True, False), (24, 5, 1, 1, True, False), (16, 3, 1, 2, False, False),
      (40, 5, 2, 1, True, True), (64, 3, 1, 1, True, True), (64, 3, 2, 1, False, False), (64, 5, 1, 1, True, False),
      (64, 7, 1, 1, False, True), (16, 7, 1, 3, True, False)]


def _dw_math(x, wt, b, s, p, dil, act, r, dt):
    """Depthwise conv: fp16 x, fp32 weights and bias as they are (misc.hip reads them as float)."""
    y = F.conv2d(_rd(x, dt), wt.to(dt), b.to(dt) if b is not None else None, s, p, dil, groups=x.shape[1])
    y = _act(y, act)
    return _rd(r, dt) + y if r is not None else y


def _dw_gpu(x, wt, b, s, p, dil, act, r):
    from ydbl.nn.modules import emit_dw

    n, c, h, w = x.shape
    k = wt.shape[2]
    ho, wo = (h + 2 * p - dil * (k - 1) - 1) // s + 1, (w + 2 * p - dil * (k - 1) - 1) // s + 1
    plan = _plan()
    xv = _tv(plan, x)
    yv = _out(plan, n, ho, wo, c)
    rv = _tv(plan, r) if r is not None else None
    emit_dw(plan, xv, yv, wt, b, s, p, dil, _act_code(act), res=rv)
    _run(plan)
    return _host(yv)


def _dw_case(c, k, s, dil, bias, res, variant):
    g = _gen(c * 100 + k * 10 + s + dil)
    n, h, w = 2, 17, 15
    x = torch.randn(n, c, h, w, generator=g)
    wt = torch.randn(c, 1, k, k, generator=g) / k
    b = torch.randn(c, generator=g) if bias or variant else None
    act = "none"
    if variant:
        b, act, sx, sw = _vary(variant, b, act, 1.0, 1.0)
        x, wt = x * sx, wt * sw
    p = dil * (k - 1) // 2
    ho, wo = (h + 2 * p - dil * (k - 1) - 1) // s + 1, (w + 2 * p - dil * (k - 1) - 1) // s + 1
    r = None
    if res and variant in (None, "large"):
        r = torch.randn(n, c, ho, wo, generator=g) * (64 if variant == "large" else 1)
    got = _dw_gpu(x, wt, b, s, p, dil, act, r)
    name = f"dw c{c} k{k} s{s} d{dil}{'/' + variant if variant else ''}"
    _check(name, got, _dw_math(x, wt, b, s, p, dil, act, r, F64), 1,
           _dw_math(x, wt, b, s, p, dil, act, r, F32).half(), variant)


@pytest.mark.parametrize("c,k,s,dil,bias,res", DW)
def test_depthwise(c, k, s, dil, bias, res):
    _dw_case(c, k, s, dil, bias, res, None)


@pytest.mark.parametrize("variant", ["large", "overflow", "tails", "small"])
@pytest.mark.parametrize("c,k", [(64, 3), (32, 5)])  # the LDS-tiled and the one-thread-per-vector kernel
def test_depthwise_value_range(c, k, variant):
    _dw_case(c, k, 1, 1, True, False, variant)


def test_depthwise_pair():
    """ydbl_dwconv2d_pair_nhwc (5x5, then 7x7 dilation 3 on the first output as stored): both outputs single-stage,
    the second against the kernel's own first output."""
    from ydbl.nn import modules as M

    torch.manual_seed(64 + 16)
    c, h, w = 64, 16, 32
    c0 = nn.Conv2d(c, c, 5, padding=2, groups=c)
    c1 = nn.Conv2d(c, c, 7, padding=9, groups=c, dilation=3)
    x = torch.randn(3, c, h, w)
    plan = _plan()
    a1, a2 = M.emit_dw_pair(plan, c0, c1, _tv(plan, x))
    assert [st.fn.__name__ for st in plan.steps] == ["ydbl_dwconv2d_pair_nhwc"]
    _run(plan)
    g1, g2 = _host(a1), _host(a2)
    w0, b0, w1, b1 = (t.detach() for t in (c0.weight, c0.bias, c1.weight, c1.bias))
    _check("dw pair, first", g1, _dw_math(x, w0, b0, 1, 2, 1, "none", None, F64), 1,
           _dw_math(x, w0, b0, 1, 2, 1, "none", None, F32).half(), None)
    _check("dw pair, second", g2, _dw_math(g1, w1, b1, 1, 9, 3, "none", None, F64), 1,
           _dw_math(g1, w1, b1, 1, 9, 3, "none", None, F32).half(), None)


# ------------------------------------------------------------------------------------------- fused dw -> pw
# The kernels with an fp16 intermediate: an intermediate that rounds the other way under another summation order
# moves the output by |w| * ulp(intermediate), an absolute amount of up to 2^-12 at these weights.  Against an output
# near zero that is several of its floored units (2^-14) whichever way the kernel sums, and the fp32 emulation
# itself then misses max|e| <= 4 (measured: 4.6 for the Detect pair, 10.4 for the box form, with N(0, 1) biases).
# So the last stage's bias is centred at +1 (+2 for the box form's activation-free 1x1): most results are of order 1,
# where the same flip is a fraction of a unit; some 5 % of the pre-activations stay negative, and both sides of SiLU
# at full strength are the single-stage cases' and the tails cases' business.  For the same reason a residual of
# these cases is N(1, 0.5^2), not N(0, 1): the sum must not cancel to near zero either.
STAGED_SHIFT = 1.0

def _dsconv_math(x, wd, bd, dw_act, wp, bp, act, r, k, s, dt):
    """dw (fp16 taps, fp32 bias, activation) -> fp16 -> pw (fp16 weights, fp32 bias, activation) [+ r]."""
    c = x.shape[1]
    mid = F.conv2d(_rd(x, dt), _rd(wd, dt), bd.to(dt) if bd is not None else None, s, k // 2, 1, groups=c)
    mid = _rd(_act(mid, dw_act), dt)
    y = _act(F.conv2d(mid, _rd(wp, dt), bp.to(dt)), act)
    return _rd(r, dt) + y if r is not None else y


# (cin, cout, k, stride, shape, residual, YDBL_DS_LEAN, the kernel the route lands on): test_dsconv_fused's and
# test_dsconv_lean_bit_identical's smallest cases per tile
DSCONV = [
    (64, 48, 5, 1, (2, 64, 11, 12), False, None, "chunked, k5"),
    (32, 32, 7, 1, (3, 32, 9, 13), False, None, "chunked, 32 channels"),
    (128, 128, 3, 2, (2, 128, 20, 20), False, "0", "chunked, stride 2"),
    (64, 64, 3, 1, (3, 64, 13, 21), True, None, "lean 64 k3, odd batch"),
    (64, 64, 7, 1, (2, 64, 9, 30), True, None, "lean 64 k7"),
    (128, 128, 3, 1, (4, 128, 20, 20), True, None, "lean 128 k3"),
    (128, 128, 3, 2, (1, 128, 19, 27), False, None, "lean 128 stride 2"),
]


def _dsconv_gpu(x, wd, bd, wp, bp, act, r, k, s, detect, tail):
    from ydbl import _lib
    from ydbl.nn import modules as M

    n, cin, h, w = x.shape
    cout = wp.shape[0]
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    dw = nn.Conv2d(cin, cin, k, s, k // 2, groups=cin, bias=False)
    with torch.no_grad():
        dw.weight.copy_(wd)
    plan = _plan()
    xv = _tv(plan, x)
    yv = _out(plan, n, ho, wo, cout)
    rv = _tv(plan, r) if r is not None else None
    tv = None
    if tail:  # the level buffer's class slice
        tv = plan.alloc(n, ho, wo, 64 + tail[0].shape[0]).cslice(64, tail[0].shape[0])
    M.emit_dsconv(plan, dw, xv, yv, wp, bp, _act_code(act), rv, _lib.RES_ADD if rv is not None else _lib.RES_NONE,
                  b_dw=bd, dw_act=_lib.ACT_SILU if detect else _lib.ACT_NONE, tail=(*tail, tv) if tail else None)
    assert [st.fn.__name__ for st in plan.steps] == ["ydbl_dsconv_nhwc"]
    _run(plan)
    return _host(yv), (_host(tv) if tv is not None else None)


def _dsconv_case(cin, cout, k, s, shape, res, lean, variant, monkeypatch, detect=False, tail=0):
    if lean is None:
        monkeypatch.delenv("YDBL_DS_LEAN", raising=False)
    else:
        monkeypatch.setenv("YDBL_DS_LEAN", lean)
    g = _gen(cin * 7 + cout + k + shape[2])
    x = torch.randn(*shape, generator=g)
    wd = torch.randn(cin, 1, k, k, generator=g) / k
    bd = 0.3 * torch.randn(cin, generator=g) if detect else None  # the Detect pair's DWConv: folded BN bias + SiLU
    wp = torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5
    bp = torch.randn(cout, generator=g) * 0.25 + STAGED_SHIFT
    act = "silu"
    if variant:  # the final stage only: the depthwise value stays at unit scale (small: 2^-9, a normal fp16)
        bp, act, sx, sw = _vary(variant, bp, act, 1.0, 1.0)
        if variant == "small":
            x, wp = x * sx, wp * sw
        else:
            wp = wp * sx
    n = shape[0]
    ho, wo = (shape[2] + 2 * (k // 2) - k) // s + 1, (shape[3] + 2 * (k // 2) - k) // s + 1
    r = None
    if res and variant in (None, "large"):
        r = (0.5 * torch.randn(n, cout, ho, wo, generator=g) + STAGED_SHIFT) * (64 if variant == "large" else 1)
    tw, tb = torch.randn(tail, cout, generator=g) / cout ** 0.5, torch.randn(tail, generator=g) + 2.0
    got, tgot = _dsconv_gpu(x, wd, bd, wp, bp, act, r, k, s, detect, (tw, tb) if tail else None)
    dwa = "silu" if detect else "none"
    name = f"dsconv {cin}->{cout} k{k} s{s}{' detect' if detect else ''}{'/' + variant if variant else ''}"
    _check(name, got, _dsconv_math(x, wd, bd, dwa, wp, bp, act, r, k, s, F64), 2,
           _dsconv_math(x, wd, bd, dwa, wp, bp, act, r, k, s, F32).half(), variant)
    if tail:  # the class conv on y as stored, fp32 weights and bias as they are: one accumulation, one rounding
        tref = F.conv2d(got.to(F64), tw.to(F64).reshape(tail, cout, 1, 1), tb.to(F64))
        temu = F.conv2d(got.float(), tw.reshape(tail, cout, 1, 1), tb).half()
        _check(name + " class tail", tgot, tref, 1, temu, None)


@pytest.mark.parametrize("cin,cout,k,s,shape,res,lean,route", DSCONV)
def test_dsconv(cin, cout, k, s, shape, res, lean, route, monkeypatch):
    _dsconv_case(cin, cout, k, s, shape, res, lean, None, monkeypatch)


@pytest.mark.parametrize("variant", ["large", "overflow", "tails", "small"])
def test_dsconv_value_range(variant, monkeypatch):
    _dsconv_case(64, 64, 3, 1, (3, 64, 13, 21), True, None, variant, monkeypatch)


@pytest.mark.parametrize("cin,cout,shape,lean", [(64, 80, (1, 64, 13, 17), None), (128, 64, (2, 128, 20, 21), None),
                                                 (64, 64, (2, 64, 40, 40), "0")])
def test_detect_dw_pw(cin, cout, shape, lean, monkeypatch):
    """The Detect DWConv -> Conv1x1 pair as one launch: dw bias + SiLU before the fp16 rounding in LDS."""
    _dsconv_case(cin, cout, 3, 1, shape, False, lean, None, monkeypatch, detect=True)


@pytest.mark.parametrize("lean", [None, "0"])
def test_detect_class_tail(lean, monkeypatch):
    """The pair plus the class conv (nc = 3) in one launch, lean and chunked tile."""
    _dsconv_case(64, 64, 3, 1, (2, 64, 40, 40), False, lean, None, monkeypatch, detect=True, tail=3)


# ------------------------------------------------------------------------------------------- Bottleneck, Detect box
def _bneck_math(x, w1, b1, w2, b2, add, w3, b3, dt):
    mid = _rd(_act(F.conv2d(_rd(x, dt), _rd(w1, dt), b1.to(dt), 1, 1), "silu"), dt)
    y = _act(F.conv2d(mid, _rd(w2, dt), b2.to(dt), 1, 1), "silu")
    if add:
        y = y + _rd(x, dt)
    if w3 is not None:
        y = F.conv2d(_rd(y, dt), _rd(w3, dt).reshape(*w3.shape, 1, 1), b3.to(dt))
    return y


def _bneck_gpu(x, w1, b1, w2, b2, add, tile_h, cs_extra, cmid, w3=None, b3=None):
    from ydbl import _lib

    n, cin, h, w = x.shape
    c = w2.shape[0]
    cm = w1.shape[0]
    plan = _plan()
    xv = _tv(plan, x, cs_extra, 0)
    if w3 is not None:
        lv = plan.alloc(n, h, w, c + 8)  # the level buffer [box 64 | cls]
        yv = lv.cslice(0, c)
        size, pack, args = _lib.lib.ydbl_detect_box_params_size(cin, c), _lib.lib.ydbl_detect_box_pack, (cin, c)
        ts = (w1, b1, w2, b2, w3, b3)
    else:
        yv = plan.alloc(n, h, w, c, cs=c + cs_extra)
        if cmid:
            size, pack, args = _lib.lib.ydbl_conv3x3_pair_params_size(c, cm), _lib.lib.ydbl_conv3x3_pair_pack, (c, cm)
        else:
            size, pack, args = _lib.lib.ydbl_bottleneck_params_size(c), _lib.lib.ydbl_bottleneck_pack, (c,)
        ts = (w1, b1, w2, b2)
    ts = [t.float().contiguous() for t in ts]
    host = torch.empty(int(size), dtype=torch.uint8)
    _lib.check(pack(*[t.data_ptr() for t in ts], *args, host.data_ptr()))
    params = host.to(DEV)
    if w3 is not None:
        d = _lib.BottleneckDesc(xv.struct(), yv.struct(), c, 0, 0, params.data_ptr(), c, 1)
    else:
        d = _lib.BottleneckDesc(xv.struct(), yv.struct(), c, int(add), tile_h, params.data_ptr(), cmid)
    plan.launch("ydbl_bottleneck_nhwc", d)
    _run(plan)
    return _host(yv)


# (c, n, h, w, add, tile_h, cs_extra, c_mid): test_bottleneck_fused cases
BNECK = [(16, 2, 64, 64, True, 0, 0, 0), (16, 2, 37, 29, False, 16, 8, 0), (32, 1, 37, 53, True, 0, 8, 0),
         (32, 2, 40, 48, False, 16, 0, 0), (64, 3, 48, 33, True, 16, 16, 0), (64, 1, 17, 100, False, 8, 0, 0),
         (64, 3, 37, 29, True, 9, 8, 0), (64, 3, 37, 29, False, 8, 8, 64)]


def _bneck_case(c, n, h, w, add, tile_h, cs_extra, cmid, variant):
    g = _gen(c * 7 + h + cmid)
    cm = cmid or c // 2
    x = torch.randn(n, c, h, w, generator=g)
    if add:  # the residual is the input itself
        x = 0.5 * x + STAGED_SHIFT
    w1 = torch.randn(cm, c, 3, 3, generator=g) / (9 * c) ** 0.5
    b1 = torch.randn(cm, generator=g) * 0.5
    w2 = torch.randn(c, cm, 3, 3, generator=g) / (9 * cm) ** 0.5
    b2 = torch.randn(c, generator=g) * 0.25 + STAGED_SHIFT
    if variant:  # the final stage only (SiLU is part of the kernel: large and tails apply)
        b2, _, sx, _ = _vary(variant, b2, "silu", 1.0, 1.0)
        w2 = w2 * sx
        add = False
    got = _bneck_gpu(x, w1, b1, w2, b2, add, tile_h, cs_extra, cmid)
    name = f"bottleneck c{c} mid{cm} {n}x{h}x{w}{' add' if add else ''}{'/' + variant if variant else ''}"
    _check(name, got, _bneck_math(x, w1, b1, w2, b2, add, None, None, F64), 2,
           _bneck_math(x, w1, b1, w2, b2, add, None, None, F32).half(), variant)


@pytest.mark.parametrize("c,n,h,w,add,tile_h,cs_extra,cmid", BNECK)
def test_bottleneck(c, n, h, w, add, tile_h, cs_extra, cmid):
    _bneck_case(c, n, h, w, add, tile_h, cs_extra, cmid, None)


@pytest.mark.parametrize("variant", ["large", "tails"])
def test_bottleneck_value_range(variant):
    _bneck_case(32, 1, 37, 53, False, 0, 8, 0, variant)


def _box_case(cin, n, h, w, cs_extra, seeds, variant):
    c = 64
    gots, refs, emus = [], [], []
    for i in range(seeds):
        g = _gen(n * 100 + h + cin + 7919 * i)
        x = torch.randn(n, cin, h, w, generator=g)
        w1, b1 = torch.randn(c, cin, 3, 3, generator=g) / (9 * cin) ** 0.5, torch.randn(c, generator=g) * 0.5
        w2, b2 = torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5, torch.randn(c, generator=g) * 0.5
        w3, b3 = torch.randn(c, c, generator=g) / c ** 0.5, torch.randn(c, generator=g) * 0.25 + 2 * STAGED_SHIFT
        if variant:  # the trailing 1x1 has no activation: large (as a scale) and overflow apply
            b3, _, sx, _ = _vary(variant, b3, "none", 1.0, 1.0)
            w3 = w3 * sx
        gots.append(_bneck_gpu(x, w1, b1, w2, b2, False, 0, cs_extra, c, w3, b3))
        refs.append(_bneck_math(x, w1, b1, w2, b2, False, w3, b3, F64))
        emus.append(_bneck_math(x, w1, b1, w2, b2, False, w3, b3, F32).half())
    name = f"detect box {cin} {n}x{h}x{w}{'/' + variant if variant else ''}"
    _check(name, torch.cat(gots), torch.cat(refs), 3, torch.cat(emus), variant)


@pytest.mark.parametrize("cin,n,h,w,cs_extra,seeds", [(64, 3, 37, 29, 8, 1), (128, 1, 3, 7, 0, 4)])
def test_detect_box(cin, n, h, w, cs_extra, seeds):
    """seeds: 128 x 1 x 3 x 7 has 1344 outputs; four draws at that shape are pooled for the >= 4096 elements."""
    _box_case(cin, n, h, w, cs_extra, seeds, None)


@pytest.mark.parametrize("variant", ["large", "overflow"])
def test_detect_box_value_range(variant):
    _box_case(64, 3, 37, 29, 8, 1, variant)


# ------------------------------------------------------------------------------------------- stem, stem2
def _stem_gpu(x, wt, b, s, act):
    n, _, h, w = x.shape
    cout = wt.shape[0]
    plan = _plan()
    yv = _out(plan, n, (h - 1) // s + 1, (w - 1) // s + 1, cout)
    xd, wd, bd = x.contiguous().to(DEV), wt.contiguous().to(DEV), b.to(DEV)
    plan.launch("ydbl_conv_stem", xd.data_ptr(), n, 3, h, w, 1.0, wd.data_ptr(), bd.data_ptr(), 3, s,
                _act_code(act), yv.struct(), None)
    _run(plan)
    return _host(yv)


def _stem_case(cout, s, h, w, variant):
    g = _gen(cout + s)
    n = 3
    x = torch.rand(n, 3, h, w, generator=g)
    wt = torch.randn(cout, 3, 3, 3, generator=g) / 27 ** 0.5 * 3.0  # the image has rms 0.58
    b = torch.randn(cout, generator=g)
    act = "silu"
    if variant:
        b, act, sx, sw = _vary(variant, b, act, 1.0, 1.0)
        x, wt = x * sx, wt * sw
    ref = _act(F.conv2d(_rd(x, F64), _rd(wt, F64), b.to(F64), s, 1), act)
    emu = _act(F.conv2d(_rd(x, F32), _rd(wt, F32), b, s, 1), act).half()
    got = _stem_gpu(x, wt, b, s, act)
    _check(f"stem {cout} s{s} {h}x{w}{'/' + variant if variant else ''}", got, ref, 1, emu, variant)


@pytest.mark.parametrize("cout,s,h,w", [(8, 1, 14, 19), (16, 2, 17, 36), (64, 2, 7, 33)])
def test_stem(cout, s, h, w):
    _stem_case(cout, s, h, w, None)


@pytest.mark.parametrize("variant", ["large", "overflow", "tails"])
def test_stem_value_range(variant):
    _stem_case(32, 1, 9, 40, variant)


def _stem2_gpu(x, w0, b0, w1, b1):
    from ydbl import _lib

    n, _, h, w = x.shape
    c0 = w0.shape[0]
    plan = _plan()
    yv = plan.alloc(n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, 2 * c0, cs=2 * c0 + 8)  # a concat slice
    host = torch.empty(int(_lib.lib.ydbl_conv_stem2_params_size(c0)), dtype=torch.uint8)
    ts = [t.float().contiguous() for t in (w0, b0, w1, b1)]
    _lib.check(_lib.lib.ydbl_conv_stem2_pack(*[t.data_ptr() for t in ts], c0, host.data_ptr()))
    params = host.to(DEV)
    xd = x.contiguous().to(DEV)
    d = _lib.Stem2Desc(xd.data_ptr(), n, 3, h, w, 1.0, c0, params.data_ptr(), yv.struct())
    plan.launch("ydbl_conv_stem2", d)
    _run(plan)
    return _host(yv)


@pytest.mark.parametrize("c0,n,h,w", [(8, 2, 64, 64), (16, 2, 37, 53)])
def test_stem2(c0, n, h, w):
    g = _gen(c0 + h)
    x = torch.rand(n, 3, h, w, generator=g)
    w0 = torch.randn(c0, 3, 3, 3, generator=g) / 27 ** 0.5 * 3.0
    b0 = torch.randn(c0, generator=g) * 0.5
    w1 = torch.randn(2 * c0, c0, 3, 3, generator=g) / (9 * c0) ** 0.5
    b1 = torch.randn(2 * c0, generator=g) * 0.25 + STAGED_SHIFT

    def math(dt):
        mid = _rd(_act(F.conv2d(_rd(x, dt), _rd(w0, dt), _rd(b0, dt), 1, 1), "silu"), dt)  # b0 as fp16: see above
        return _act(F.conv2d(mid, _rd(w1, dt), b1.to(dt), 2, 1), "silu")

    ref = math(F64)
    got = _stem2_gpu(x, w0, b0, w1, b1)
    _check(f"stem2 c{c0} {n}x{h}x{w}", got, ref, 2, math(F32).half(), None)
