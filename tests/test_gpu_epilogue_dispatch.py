"""The conv / DSConv epilogues decide their form (activation, residual mode) once per wave, or once per launch
on the host (csrc/common.hpp with_act, csrc/conv_common.hpp conv_epilogue): one small launch per kernel family
that shares the epilogue, crossed with activation x residual mode.  Each case must equal the runtime-dispatch
form (YDBL_EPI_GENERIC=1) bit for bit, and stay within the existing test_conv_* / test_dsconv_* fp16 bound of
the fp32 torch reference (rtol = atol = 2e-2 for the dense convs, 3e-2 for the DSConv launches).
"""

import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops import _plan, _run, _tv_from_nchw

pytestmark = pytest.mark.gpu

ACTS = ["none", "silu", "gelu", "sigmoid"]
RESS = [None, "add", "mul"]
DENSE_TOL = dict(rtol=2e-2, atol=2e-2)  # test_gpu_ops._tol(fp16)
DS_TOL = dict(rtol=3e-2, atol=3e-2)     # test_dsconv_lean_bit_identical / test_detect_cls_tail_fused

# family -> (cin, cout, k, stride, n, h, w)
DENSE = {
    "igemm_1x1_64_64": (64, 64, 1, 1, 2, 9, 13),
    "igemm_1x1_64_66": (64, 66, 1, 1, 2, 9, 13),       # Cout % 4 != 0: the form with per-channel tails
    "conv3x3_16_32_s1": (16, 32, 3, 1, 1, 17, 19),
    "conv3x3_16_32_s2": (16, 32, 3, 2, 1, 17, 19),
    "tile3x3_16_32_s1": (16, 32, 3, 1, 1, 64, 72),     # >= 4096 output pixels: the spatial-tile kernel
    "tile3x3_16_32_s2": (16, 32, 3, 2, 1, 128, 128),
    "halo3x3_64_64": (64, 64, 3, 1, 1, 160, 160),      # the smallest map the halo kernel takes unsplit
    "halo3x3_split_256_64": (256, 64, 3, 1, 1, 64, 64),
    "wsk_1x1_512_64": (512, 64, 1, 1, 2, 8, 8),
}


def _act_code(act):
    from ydbl import _lib

    return {"none": _lib.ACT_NONE, "silu": _lib.ACT_SILU, "gelu": _lib.ACT_GELU, "sigmoid": _lib.ACT_SIGMOID}[act]


def _res_code(res):
    from ydbl import _lib

    return {None: _lib.RES_NONE, "add": _lib.RES_ADD, "mul": _lib.RES_MUL}[res]


def _act_ref(v, act):
    return {"none": lambda t: t, "silu": F.silu, "gelu": F.gelu, "sigmoid": torch.sigmoid}[act](v)


def _with_res(v, r, res):
    r = r.half().float()
    return v if res is None else r + v if res == "add" else r * v


@functools.lru_cache(maxsize=None)
def _dense_inputs(family):
    """Inputs and the fp32 pre-activation reference of a family, computed once for all its cases."""
    cin, cout, k, s, n, h, w = DENSE[family]
    g = torch.Generator().manual_seed(sum(map(ord, family)))
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g)
    pre = F.conv2d(x.half().float(), wt.half().float(), b, s, k // 2)
    r = torch.randn(*pre.shape, generator=g)
    r2 = torch.randn(*pre.shape, generator=g)
    return x, wt, b, pre, r, r2


def _run_dense(family, act, res, sliced=False, second=False):
    from ydbl.nn.modules import emit_dense

    cin, cout, k, s, n, h, w = DENSE[family]
    x, wt, b, pre, r, r2 = _dense_inputs(family)
    plan = _plan(torch.float16)
    xv = _tv_from_nchw(plan, x)
    ho, wo = pre.shape[2:]
    yv = plan.alloc(n, ho, wo, cout + 16).cslice(8, cout) if sliced else plan.alloc(n, ho, wo, cout)
    rv = _tv_from_nchw(plan, r) if res else None
    emit_dense(plan, xv, yv, wt, b, s, k // 2, 1, _act_code(act), rv, _res_code(res))
    y2 = None
    if second:  # FullPAD second output y2 = 0.5 * y + r2
        y2 = plan.alloc(n, ho, wo, cout)
        assert plan.fuse_second_output(plan.writer_of(yv), y2, _tv_from_nchw(plan, r2), 0.5, 1.0) is not None
    _run(plan)
    return yv.nchw().float().cpu(), (y2.nchw().float().cpu() if second else None)


def _check_dense(monkeypatch, family, act, res, sliced=False, second=False):
    outs = []
    for generic in ("0", "1"):
        monkeypatch.setenv("YDBL_EPI_GENERIC", generic)
        outs.append(_run_dense(family, act, res, sliced, second))
    assert torch.equal(outs[0][0], outs[1][0]), (outs[0][0] - outs[1][0]).abs().max()
    _, _, _, pre, r, r2 = _dense_inputs(family)
    want = _with_res(_act_ref(pre, act), r, res)
    torch.testing.assert_close(outs[0][0], want, **DENSE_TOL)
    if second:
        assert torch.equal(outs[0][1], outs[1][1])
        torch.testing.assert_close(outs[0][1], 0.5 * outs[0][0] + r2.half().float(), **DENSE_TOL)


@pytest.mark.parametrize("res", RESS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("family", list(DENSE))
def test_dense_epilogue_forms(monkeypatch, family, act, res):
    _check_dense(monkeypatch, family, act, res)


@pytest.mark.parametrize("family", ["igemm_1x1_64_64", "tile3x3_16_32_s1", "halo3x3_64_64", "wsk_1x1_512_64"])
def test_dense_epilogue_sliced_output(monkeypatch, family):
    _check_dense(monkeypatch, family, "silu", "add", sliced=True)


@pytest.mark.parametrize("family", ["igemm_1x1_64_64", "tile3x3_16_32_s1", "halo3x3_64_64", "wsk_1x1_512_64"])
def test_dense_epilogue_second_output(monkeypatch, family):
    _check_dense(monkeypatch, family, "silu", "add", second=True)


# ---- DSConv (chunked and lean) and the Detect pair with the class tail -------------------------------------
@functools.lru_cache(maxsize=None)
def _ds_inputs(kind):
    n, h, w = (1, 11, 13) if kind == "tail" else (3, 9, 13)
    g = torch.Generator().manual_seed(11 if kind == "tail" else 7)
    x = torch.randn(n, 64, h, w, generator=g)
    wdw = torch.randn(64, 1, 3, 3, generator=g) / 3
    bdw = torch.randn(64, generator=g) * 0.2
    wpw = torch.randn(64, 64, 1, 1, generator=g) / 8
    bpw = torch.randn(64, generator=g) * 0.2
    wt = torch.randn(3, 64, generator=g) / 8
    bt = torch.randn(3, generator=g) * 0.2
    r = torch.randn(n, 64, h, w, generator=g)
    dw = F.conv2d(x.half().float(), wdw.half().float(), None, 1, 1, 1, 64)  # taps rounded to fp16, fp32 sums
    return x, wdw, bdw, wpw, bpw, wt, bt, r, dw


def _ds_ref(kind, act, res):
    x, wdw, bdw, wpw, bpw, wt, bt, r, dw = _ds_inputs(kind)
    if kind == "tail":  # DWConv: bias + the same activation before the pointwise
        dw = _act_ref(dw + bdw.view(1, -1, 1, 1), act)
    y = _act_ref(F.conv2d(dw.half().float(), wpw.half().float(), bpw), act)
    y = _with_res(y, r, res)
    t = F.conv2d(y.half().float(), wt.view(3, 64, 1, 1), bt) if kind == "tail" else None
    return y, t


def _run_ds(kind, act, res):
    from ydbl.nn.modules import emit_dsconv

    x, wdw, bdw, wpw, bpw, wt, bt, r, _ = _ds_inputs(kind)
    n, _, h, w = x.shape
    plan = _plan(torch.float16)
    xv = _tv_from_nchw(plan, x)
    yv = plan.alloc(n, h, w, 64)
    rv = _tv_from_nchw(plan, r) if res else None
    conv = torch.nn.Conv2d(64, 64, 3, 1, 1, groups=64, bias=False)
    tv = None
    if kind == "tail":
        tv = plan.alloc(n, h, w, 3)
        emit_dsconv(plan, conv, xv, yv, wpw, bpw, _act_code(act), w_dw=wdw, b_dw=bdw, dw_act=_act_code(act),
                    tail=(wt, bt, tv))
    else:
        emit_dsconv(plan, conv, xv, yv, wpw, bpw, _act_code(act), rv, _res_code(res), w_dw=wdw)
    _run(plan)
    return yv.nchw().float().cpu(), (tv.nchw().float().cpu() if tv is not None else None)


def _check_ds(monkeypatch, kind, lean, act, res):
    monkeypatch.setenv("YDBL_DS_LEAN", lean)
    outs = []
    for generic in ("0", "1"):
        monkeypatch.setenv("YDBL_EPI_GENERIC", generic)
        outs.append(_run_ds(kind, act, res))
    assert torch.equal(outs[0][0], outs[1][0]), (outs[0][0] - outs[1][0]).abs().max()
    y, t = _ds_ref(kind, act, res)
    torch.testing.assert_close(outs[0][0], y, **DS_TOL)
    if t is not None:
        assert torch.equal(outs[0][1], outs[1][1])
        torch.testing.assert_close(outs[0][1], t, **DS_TOL)


@pytest.mark.parametrize("res", RESS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("lean", ["1", "0"])
def test_dsconv_epilogue_forms(monkeypatch, lean, act, res):
    """64 -> 64 k3 DSConv, N=3, 9x13: the lean tile (YDBL_DS_LEAN=1) and the chunked kernel."""
    _check_ds(monkeypatch, "ds", lean, act, res)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("lean", ["1", "0"])
def test_detect_pair_tail_epilogue_forms(monkeypatch, lean, act):
    """Detect DWConv -> Conv1x1 pair with the 3-class tail, N=1, 11x13 (the tail takes no residual)."""
    _check_ds(monkeypatch, "tail", lean, act, None)


def test_fp32_parity_silu_is_exact_form():
    """The fp32 parity path keeps x / (1 + exp(-x)) (IEEE exp and division), not the fp16 paths' fast form."""
    from ydbl import _lib
    from ydbl.nn.modules import emit_dense

    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 9, 13, generator=g)
    wt = torch.randn(64, 64, 1, 1, generator=g) / 8
    b = torch.randn(64, generator=g)
    plan = _plan(torch.float32)
    xv = _tv_from_nchw(plan, x)
    yv = plan.alloc(2, 9, 13, 64)
    emit_dense(plan, xv, yv, wt, b, 1, 0, 1, _lib.ACT_SILU)
    _run(plan)
    pre = F.conv2d(x, wt, b)
    want = pre / (1 + torch.exp(-pre))
    torch.testing.assert_close(yv.nchw().float().cpu(), want, rtol=2e-5, atol=2e-5)  # test_gpu_ops._tol(fp32)
