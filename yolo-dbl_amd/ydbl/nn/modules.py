"""YOLO-DBL building blocks, MI355X path.

Each class keeps the reference's constructor signature, submodule names and
parameter shapes (so ``parse_model`` resolves the DBL YAMLs by class name and
reference ``state_dict`` keys load unchanged).  Its compute is ``emit``: HIP
launches appended to a ``Plan``:

    y = module.emit(plan, x, out=None)   # x, y: NHWC TV views (lists for multi-input)

and its ``forward(x)`` (the reference's module contract, ``m(x)`` on a tensor or a
list of tensors, U/nn/tasks.py:158-161) compiles that emit into a one-module plan
for x's shapes / dtype / device, caches it, and runs it (``run_module``).  A
registered plugin class WITHOUT ``emit`` -- a plain torch ``forward`` -- runs
inside the model's plan as a captured torch step on NCHW views of its input
(``emit_torch``).

``out`` (optional) is a destination view, typically a channel slice of a
concat buffer, so Concat / chunk / C2f / C3 concatenations cost no copies.
BatchNorm is folded exactly as ``fuse_conv_and_bn`` does
(U/utils/torch_utils.py:238-265); DSConv's BN (left unfused by the reference,
U/nn/tasks.py:217) is folded into its pointwise conv here.
"""

from __future__ import annotations

import copy
import math
import os

import torch
import torch.nn as nn

from .. import _lib
from .._lib import ConvDesc, DwConvDesc, HgDesc, View
from ..runtime import TV, Plan, Step, round_up, weights_signature, ydbl_env
from ..tail import CandidateLists, E2ETail, decode_desc


# =============================================================================== weight prep + launches
def autopad(k, p=None, d=1):
    """U/nn/modules/conv.py:30-36."""
    if d > 1:
        k = d * (k - 1) + 1 if isinstance(k, int) else [d * (x - 1) + 1 for x in k]
    if p is None:
        p = k // 2 if isinstance(k, int) else [x // 2 for x in k]
    return p


@torch.no_grad()
def fold_bn(weight: torch.Tensor, bias: torch.Tensor | None, bn: nn.BatchNorm2d):
    """Same op sequence as fuse_conv_and_bn (diag-matrix products), fp32 on the host."""
    w = weight.detach().float().cpu()
    co = w.shape[0]
    w_bn = torch.diag(bn.weight.detach().float().cpu().div(torch.sqrt(bn.eps + bn.running_var.float().cpu())))
    wf = torch.mm(w_bn, w.view(co, -1)).view(w.shape)
    b_conv = torch.zeros(co) if bias is None else bias.detach().float().cpu()
    b_bn = bn.bias.detach().float().cpu() - bn.weight.detach().float().cpu().mul(
        bn.running_mean.float().cpu()
    ).div(torch.sqrt(bn.running_var.float().cpu() + bn.eps))
    bf = torch.mm(w_bn, b_conv.reshape(-1, 1)).reshape(-1) + b_bn
    return wf, bf


def _act_code(act) -> int:
    if isinstance(act, nn.SiLU):
        return _lib.ACT_SILU
    if isinstance(act, nn.GELU):
        return _lib.ACT_GELU
    if isinstance(act, nn.Identity) or act is None:
        return _lib.ACT_NONE
    raise NotImplementedError(f"activation {type(act).__name__} has no HIP epilogue")


def vec_aligned(v: TV) -> bool:
    """The 16-byte channel-vector rule of check_view(need_vec_align) (csrc/capi.hip): channel count, channel
    stride and base pointer all in whole 16-byte vectors."""
    vec = 16 // v.base.element_size()
    return v.c % vec == 0 and v.cs % vec == 0 and v.ptr % 16 == 0


def _null_view() -> View:
    return View(None, 0, 0, 0, 0, 0, 0)


def emit_dense(plan: Plan, x: TV, y: TV, w: torch.Tensor, b: torch.Tensor | None, stride=1, pad=0, dil=1,
               act=_lib.ACT_NONE, res: TV | None = None, res_mode=_lib.RES_NONE, what="conv"):
    """Dense conv y = act(conv(x) + b) [+/* res]; w fp32 [co, ci, kh, kw] (ci may be < x.c: zero-padded)."""
    co, ci, kh, kw = w.shape
    assert ci <= x.c and co == y.c, (w.shape, x.shape, y.shape)
    wt = w.permute(0, 2, 3, 1)
    if ci < x.c:
        wt = torch.nn.functional.pad(wt, (0, x.c - ci))
    K = kh * kw * x.c
    kpad = round_up(K, 32)
    wk32 = torch.nn.functional.pad(wt.reshape(co, K).float(), (0, kpad - K))
    wd = plan.const(wk32.to(plan.dtype))
    bd = plan.const(b.float()) if b is not None else None
    d = ConvDesc(x.struct(), y.struct(), res.struct() if res is not None else _null_view(), wd.data_ptr(),
                 bd.data_ptr() if bd is not None else None, kh, kw, stride, pad, dil, kpad, act, res_mode,
                 _null_view(), _null_view(), 0.0, 0.0, None, 1.0)
    ws = None
    if plan.device.type != "meta":  # split-K scratch of the deep-K small-map convs (include/ydbl.h ydbl_conv_workspace)
        nws = int(_lib.lib.ydbl_conv_workspace(d))
        if nws > 0:
            ws = plan.splitk_scratch(nws)
            d.workspace, d.workspace_bytes = ws.data_ptr(), nws
    plan.launch("ydbl_conv2d_nhwc", d, what=what, keep=[wd, bd, d, ws])
    plan.note_writer(y, d)
    if plan.dtype == torch.float16 and x.c >= 64 and not what.startswith("Detect."):
        d._b32 = b.detach().float().cpu() if b is not None else None  # (ydbl.quant's bias correction)
        plan.fp8_candidates.append((d, x, wk32))  # see ydbl.quant: e4m3 operands after calibration
        plan.fp8_layers.append(getattr(plan, "cur_layer", -1))


def dw_desc(plan: Plan, x: TV, y: TV, w: torch.Tensor, b: torch.Tensor | None, stride=1, pad=0, dil=1,
            act=_lib.ACT_NONE, res: TV | None = None):
    """Depthwise conv descriptor (+ the device constants it points at); w fp32 [c, 1, kh, kw]."""
    c, _, kh, kw = w.shape
    assert c == x.c == y.c
    wd = plan.const(w.float().reshape(c, kh * kw).t().contiguous())
    bd = plan.const(b.float()) if b is not None else None
    d = DwConvDesc(x.struct(), y.struct(), res.struct() if res is not None else _null_view(), wd.data_ptr(),
                   bd.data_ptr() if bd is not None else None, kh, kw, stride, pad, dil, act,
                   _lib.RES_ADD if res is not None else _lib.RES_NONE)
    return d, [wd, bd, d]


def emit_dw(plan: Plan, x: TV, y: TV, w: torch.Tensor, b: torch.Tensor | None, stride=1, pad=0, dil=1,
            act=_lib.ACT_NONE, res: TV | None = None, what="dwconv"):
    """Depthwise conv; w fp32 [c, 1, kh, kw]."""
    d, keep = dw_desc(plan, x, y, w, b, stride, pad, dil, act, res)
    plan.launch("ydbl_dwconv2d_nhwc", d, what=what, keep=keep)


def emit_dw_pair(plan: Plan, c0: nn.Conv2d, c1: nn.Conv2d, x: TV, what="dw_pair") -> tuple[TV, TV]:
    """Two chained depthwise nn.Conv2d (c1 reads c0's output) as one ydbl_dwconv2d_pair_nhwc launch
    (the library falls back to two launches for geometries it does not fuse)."""
    descs, keep = [], []
    src, outs = x, []
    for conv in (c0, c1):
        k, s, p, d = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
        ho, wo = conv_out_hw(src.h, src.w, k, s, p, d)
        y = plan.alloc(src.n, ho, wo, conv.out_channels)
        b = conv.bias.detach().float().cpu() if conv.bias is not None else None
        dd, kk = dw_desc(plan, src, y, conv.weight.detach().float().cpu(), b, s, p, d)
        descs.append(dd)
        keep += kk
        outs.append(y)
        src = y
    plan.launch("ydbl_dwconv2d_pair_nhwc", descs[0], descs[1], what=what, keep=keep)
    return outs[0], outs[1]


def conv_out_hw(h, w, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1, (w + 2 * p - d * (k - 1) - 1) // s + 1


def emit_conv2d(plan: Plan, conv: nn.Conv2d, x: TV, out: TV | None, weight=None, bias=None, act=_lib.ACT_NONE,
                res: TV | None = None, res_mode=_lib.RES_NONE, what="conv") -> TV:
    """Launch an nn.Conv2d (dense or depthwise) with optional replacement weight/bias."""
    k, s, p, d = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
    assert conv.kernel_size[0] == conv.kernel_size[1] and conv.stride[0] == conv.stride[1]
    w = (conv.weight if weight is None else weight).detach().float().cpu()
    b = bias if bias is not None else (conv.bias.detach().float().cpu() if conv.bias is not None else None)
    ho, wo = conv_out_hw(x.h, x.w, k, s, p, d)
    y = out if out is not None else plan.alloc(x.n, ho, wo, conv.out_channels)
    assert (y.h, y.w, y.c) == (ho, wo, conv.out_channels), ((y.h, y.w, y.c), (ho, wo, conv.out_channels))
    if conv.groups == 1:
        emit_dense(plan, x, y, w, b, s, p, d, act, res, res_mode, what)
    elif conv.groups == conv.in_channels == conv.out_channels:
        if res_mode not in (_lib.RES_NONE, _lib.RES_ADD):
            raise NotImplementedError("depthwise conv supports residual ADD only")
        emit_dw(plan, x, y, w, b, s, p, d, act, res if res_mode == _lib.RES_ADD else None, what)
    elif conv.in_channels % conv.groups == 0 and conv.out_channels % conv.groups == 0 and x.c == conv.in_channels:
        emit_grouped(plan, x, y, w, b, conv.groups, s, p, d, act, res, res_mode, what)
    else:
        raise NotImplementedError(f"grouped conv g={conv.groups} with {x.c} -> {conv.out_channels} channels")
    return y


def emit_grouped(plan: Plan, x: TV, y: TV, w: torch.Tensor, b: torch.Tensor | None, groups: int, stride=1, pad=0,
                 dil=1, act=_lib.ACT_NONE, res: TV | None = None, res_mode=_lib.RES_NONE, what="conv"):
    """Grouped dense conv (1 < groups < cin; yolov13.yaml's Conv [.., 3, 2, 1, g]); w fp32 [co, ci/groups, kh, kw].
    One dense launch per group on channel slices of x, y (and res) with that group's weight rows, when every slice
    keeps the dense entry point's rules (16-byte channel vectors, cin % 8); else one dense launch with
    block-diagonal, zero-filled weights.  The same sums either way.  A per-group launch registers its own slice
    as written (note_writer), never y: a FullPAD_Tunnel on y then takes its own launch."""
    co, cig = w.shape[0], w.shape[1]
    cog = co // groups
    xs = [x.cslice(i * cig, cig) for i in range(groups)]
    ys = [y.cslice(i * cog, cog) for i in range(groups)]
    rs = [res.cslice(i * cog, cog) if res is not None else None for i in range(groups)]
    if cig % 8 == 0 and all(vec_aligned(v) for v in (*xs, *ys, *(r for r in rs if r is not None))):
        for i in range(groups):
            rows = slice(i * cog, (i + 1) * cog)
            emit_dense(plan, xs[i], ys[i], w[rows], b[rows] if b is not None else None, stride, pad, dil, act, rs[i],
                       res_mode, f"{what}.g{i}/{groups}")
        return
    full = torch.zeros((co, cig * groups, *w.shape[2:]), dtype=w.dtype)
    for i in range(groups):
        full[i * cog:(i + 1) * cog, i * cig:(i + 1) * cig] = w[i * cog:(i + 1) * cog]
    emit_dense(plan, x, y, full, b, stride, pad, dil, act, res, res_mode, f"{what}.g{groups}dense")


def fused_dsconv_ok(dw: nn.Conv2d, x: TV, dtype) -> bool:
    k, st, d = dw.kernel_size[0], dw.stride[0], dw.dilation[0]
    cc = 32 if dtype == torch.float16 else 16
    return (dw.kernel_size[0] == dw.kernel_size[1] and (k, st, d) in ((3, 1, 1), (3, 2, 1), (5, 1, 1), (7, 1, 1))
            and x.c % cc == 0 and x.c == dw.in_channels)


def emit_dsconv(plan: Plan, dw: nn.Conv2d, x: TV, out: TV | None, w_pw: torch.Tensor, b_pw: torch.Tensor,
                act=_lib.ACT_SILU, res: TV | None = None, res_mode=_lib.RES_NONE, what="DSConv",
                w_dw: torch.Tensor | None = None, b_dw: torch.Tensor | None = None, dw_act=_lib.ACT_NONE,
                tail: tuple | None = None, y_unused: bool = False) -> TV:
    """DSConv (conv.py:91-108) as one ydbl_dsconv_nhwc launch: depthwise tile in LDS feeding the pw MFMA.
    w_dw / b_dw / dw_act: folded DWConv weights, bias and activation (Detect's DWConv -> Conv1x1 pair).
    tail = (w [n, co], b [n], out view): a trailing 1x1 conv with n <= 4 outputs in the same launch.
    y_unused (with tail): nothing reads y, the launch may leave it unwritten (include/ydbl.h)."""
    k, st, p, d = dw.kernel_size[0], dw.stride[0], dw.padding[0], dw.dilation[0]
    c = x.c
    co = w_pw.shape[0]
    ho, wo = conv_out_hw(x.h, x.w, k, st, p, d)
    y = out if out is not None else plan.alloc(x.n, ho, wo, co)
    assert (y.h, y.w, y.c) == (ho, wo, co), ((y.h, y.w, y.c), (ho, wo, co))
    wdw = (dw.weight if w_dw is None else w_dw).detach().float().cpu()
    dww = plan.const(wdw.reshape(c, k * k).t().contiguous())
    kpad = round_up(c, 32)
    pww = plan.const(torch.nn.functional.pad(w_pw.reshape(co, c).float(), (0, kpad - c)).to(plan.dtype))
    bd = plan.const(b_pw.float())
    dwb = plan.const(b_dw.float()) if b_dw is not None else None
    tw = tb = None
    tail_args = (None, None, _null_view(), 0)
    if tail is not None:
        tw, tb = plan.const(tail[0].float().contiguous()), plan.const(tail[1].float().contiguous())
        tail_args = (tw.data_ptr(), tb.data_ptr(), tail[2].struct(), tail[2].c)
        what += "+1x1"
    desc = _lib.DsConvDesc(x.struct(), y.struct(), res.struct() if res is not None else _null_view(),
                           dww.data_ptr(), pww.data_ptr(), bd.data_ptr(), k, st, p, d, kpad, act, res_mode,
                           dwb.data_ptr() if dwb is not None else None, dw_act, *tail_args)
    desc.y_unused = int(bool(y_unused and tail is not None))
    plan.launch("ydbl_dsconv_nhwc", desc, what=f"{what}.k{k}s{st}", keep=[dww, pww, bd, dwb, tw, tb, desc])
    return y


def emit_dw_pw(plan: Plan, dwc: "DWConv", pwc: "Conv", x: TV, out: TV | None = None, what="DWConv+Conv1x1",
               tail_conv: nn.Conv2d | None = None, tail_out: TV | None = None, y_unused: bool = False):
    """nn.Sequential(DWConv(c, c, k), Conv(c, c2, 1)) of the Detect head (head.py:93-101): one fused launch
    when the shapes allow (the depthwise output stays in LDS), else two.  With tail_conv (the class conv
    cv3[i][2], 1x1 c2 -> nc, bias) the launch also writes tail_out when c2 == 64 and nc <= 4; returns
    (y, tail_done).  y_unused: the caller reads only tail_out, so a launch that fuses the tail need not write y."""
    if (fused_dsconv_ok(dwc.conv, x, plan.dtype) and pwc.conv.kernel_size == (1, 1) and pwc.conv.stride == (1, 1)
            and dwpw_fuse(pwc.conv.out_channels)):
        wd, bdw = dwc.folded()
        wp, bp = pwc.folded()
        if bdw is None:
            bdw = torch.zeros(x.c)
        tail = None
        if (tail_conv is not None and not os.environ.get("YDBL_NO_CLS_TAIL") and wp.shape[0] == 64
                and tail_conv.kernel_size == (1, 1) and tail_conv.groups == 1
                and tail_conv.in_channels == 64 and 1 <= tail_conv.out_channels <= 4 and tail_conv.bias is not None):
            nc = tail_conv.out_channels
            tail = (tail_conv.weight.detach().float().reshape(nc, 64), tail_conv.bias.detach().float(), tail_out)
        y = emit_dsconv(plan, dwc.conv, x, out, wp, bp if bp is not None else torch.zeros(wp.shape[0]),
                        _act_code(pwc.act), what=what, w_dw=wd, b_dw=bdw, dw_act=_act_code(dwc.act), tail=tail,
                        y_unused=y_unused)
        return y, tail is not None
    return pwc.emit(plan, dwc.emit(plan, x), out), False


def dwpw_fuse(c2: int) -> bool:
    """Whether the Detect DWConv -> Conv1x1 pair runs as one launch: at 64 pointwise outputs (DBL-n) the fused pair
    is faster (separate: DBL-n bs32 -1.8 %), at 128 and more (DBL-s / DBL-l) the two launches are (DBL-s bs8 +1.1 %,
    bs64 +2.0 %, DBL-l 1280 bs8 +1.9 %: profiles/r06/r06_detect_switch_sweep.txt).  YDBL_DWPW=1 / 0 forces either."""
    e = os.environ.get("YDBL_DWPW")
    return e == "1" or (e is None and c2 <= 64)


def stem_ok(m, ch: int) -> bool:
    """The first layer can run as ydbl_conv_stem (3x3 Conv on the raw NCHW image)."""
    if type(m) is not Conv:
        return False
    c = m.conv
    return (c.groups == 1 and c.in_channels == ch and ch == 3 and c.kernel_size == (3, 3)
            and c.padding == (1, 1) and c.dilation == (1, 1) and c.stride[0] == c.stride[1] in (1, 2)
            and c.out_channels % 4 == 0 and c.out_channels <= 64 and isinstance(m.act, (nn.SiLU, nn.Identity)))


def emit_stem(m: "Conv", plan: Plan, x_nchw: torch.Tensor, n: int, ch: int, h: int, w: int, bind=None) -> TV:
    """preprocess (U/engine/predictor.py:116-134) + first Conv (conv.py:39-63, BN folded) in one kernel.
    bind: an _lib.InputBind (the batch pointer / LoadTensor maximum read when the plan runs) or None."""
    wf, bf = m.folded()
    s = m.conv.stride[0]
    ho, wo = conv_out_hw(h, w, 3, s, 1, 1)
    y = plan.alloc(n, ho, wo, m.conv.out_channels)
    wd = plan.const(wf.float().contiguous())
    bd = plan.const((bf if bf is not None else torch.zeros(m.conv.out_channels)).float())
    plan.launch("ydbl_conv_stem", x_nchw.data_ptr(), n, ch, h, w, 1.0, wd.data_ptr(), bd.data_ptr(), 3, s,
                _act_code(m.act), y.struct(), bind, what="Stem.conv3x3", keep=[wd, bd, bind])
    return y


def stem2_ok(m0, m1, ch: int, dtype) -> bool:
    """Layers 0-1 can run as ydbl_conv_stem2: Conv(3, C0, 3, 1) + Conv(C0, 2*C0, 3, 2), SiLU, fp16, C0 in {8, 16}."""
    if dtype != torch.float16 or not stem_ok(m0, ch) or type(m1) is not Conv:
        return False
    a, b = m0.conv, m1.conv
    return (a.stride == (1, 1) and a.out_channels in (8, 16) and isinstance(m0.act, nn.SiLU)
            and isinstance(m1.act, nn.SiLU) and b.groups == 1 and b.in_channels == a.out_channels
            and b.out_channels == 2 * a.out_channels and b.kernel_size == (3, 3) and b.stride == (2, 2)
            and b.padding == (1, 1) and b.dilation == (1, 1) and m1.f == -1)


def emit_stem2(m0: "Conv", m1: "Conv", plan: Plan, x_nchw: torch.Tensor, n: int, ch: int, h: int, w: int,
               out: TV | None = None, bind=None) -> TV:
    """preprocess + layers 0 and 1 (conv.py:39-63, BN folded) in one kernel; layer 0's map stays in LDS.
    bind: an _lib.InputBind or None (emit_stem)."""
    w0, b0 = m0.folded()
    w1, b1 = m1.folded()
    c0 = m0.conv.out_channels
    ho, wo = conv_out_hw(h, w, 3, 2, 1, 1)
    y = out if out is not None else plan.alloc(n, ho, wo, 2 * c0)
    b0 = b0 if b0 is not None else torch.zeros(c0)
    b1 = b1 if b1 is not None else torch.zeros(2 * c0)
    host = torch.empty(int(_lib.lib.ydbl_conv_stem2_params_size(c0)), dtype=torch.uint8)
    args = [t.float().contiguous() for t in (w0, b0, w1, b1)]
    _lib.check(_lib.lib.ydbl_conv_stem2_pack(*[t.data_ptr() for t in args], c0, host.data_ptr()), "ydbl_conv_stem2_pack")
    params = plan.const(host)
    d = _lib.Stem2Desc(x_nchw.data_ptr(), n, ch, h, w, 1.0, c0, params.data_ptr(), y.struct(),
                       bind if bind is not None else _lib.InputBind())
    plan.launch("ydbl_conv_stem2", d, what="Stem.conv3x3x2", keep=[params, d])
    return y


def emit_merged(plan: Plan, convs, x: TV, out: TV, what="Conv1x1x2") -> TV:
    """Several Convs that read the same x with the same kernel/stride/activation as ONE launch: the
    folded weights/biases are concatenated along the output channels, in order, into `out`
    (channel slices of one buffer), e.g. C3's cv2 and cv1 (U/nn/modules/block.py:259-273)."""
    ws, bs = zip(*(m.folded() for m in convs))
    c0 = convs[0].conv
    k, st, pd, dl = c0.kernel_size[0], c0.stride[0], c0.padding[0], c0.dilation[0]
    assert (out.h, out.w, out.c) == (*conv_out_hw(x.h, x.w, k, st, pd, dl), sum(w.shape[0] for w in ws))
    emit_dense(plan, x, out, torch.cat(ws, 0), torch.cat(bs, 0), st, pd, dl, _act_code(convs[0].act), what=what)
    return out


def mergeable(convs) -> bool:
    a = convs[0]
    return all(type(m) is Conv and m.conv.kernel_size == a.conv.kernel_size and m.conv.stride == a.conv.stride
               and m.conv.padding == a.conv.padding and m.conv.groups == 1 == a.conv.groups
               and m.conv.dilation == a.conv.dilation and type(m.act) is type(a.act) for m in convs)


def emit_seq(plan: Plan, mods, x, out=None):
    mods = list(mods)
    for i, m in enumerate(mods):
        x = emit_module(m, plan, x, out if i == len(mods) - 1 else None)
    return x


def emit_copy(plan: Plan, src: TV, dst: TV):
    plan.launch("ydbl_pool_up_concat", None, src.struct(), None, dst.struct(), what="copy")


# =============================================================================== module-level forward(x)
def _check_input(t, dev=None, dt=None):
    if not isinstance(t, torch.Tensor) or t.ndim != 4:
        raise TypeError(f"expected BCHW tensors, got {type(t).__name__} {getattr(t, 'shape', '')}")
    if t.device.type != "cuda":
        raise RuntimeError(f"ydbl runs on MI355X (gfx950) only: input on {t.device}, move it to a cuda device")
    if t.dtype not in (torch.float32, torch.float16):
        raise TypeError(f"input dtype {t.dtype}: float32 or float16 (half) expected")
    if (dev is not None and t.device != dev) or (dt is not None and t.dtype != dt):
        raise ValueError("all inputs of one module call must share device and dtype")


class _ModulePlan:
    """One compiled forward of one module for one input signature: input views the call copies into, the plan,
    and the function that turns the plan's outputs into fresh NCHW tensors."""

    def __init__(self, m, xs, multi):
        dev, dt = xs[0].device, xs[0].dtype
        self.plan = Plan(dev, dt)
        self.views = [self.plan.alloc(t.shape[0], t.shape[2], t.shape[3], t.shape[1]) for t in xs]
        inp = self.views if multi else self.views[0]
        self.finish = m._forward_plan(self.plan, inp) if hasattr(m, "_forward_plan") else _tensor_out(
            emit_module(m, self.plan, inp))
        self.wsig = weights_signature(m)

    def __call__(self, xs):
        with torch.no_grad():
            for v, t in zip(self.views, xs):
                v.torch().copy_(t.permute(0, 2, 3, 1))  # NCHW -> the plan's NHWC input buffer
        self.plan.run()
        return self.finish()


def _tensor_out(y):
    if isinstance(y, (list, tuple)):
        return lambda: [v.nchw().contiguous() for v in y]
    return lambda: y.nchw().contiguous()


def run_module(m: nn.Module, x):
    """forward(x) of a built-in module: x a BCHW cuda tensor (or a list for Concat / FullPAD_Tunnel / HyperACE /
    FuseModule / Detect) in fp32 or fp16 (the half path); returns fresh NCHW tensors of x's dtype.  The module's
    emit is compiled once per (input shapes, dtype, device, YDBL_* switches) into a plan with its own buffers (the
    two most recent kept) and rebuilt when the module's weights change (runtime.weights_signature, checked after
    the launch).  BN is folded: inference semantics, as the reference after fuse()."""
    multi = isinstance(x, (list, tuple))
    xs = list(x) if multi else [x]
    if not xs:
        raise ValueError("no inputs")
    for t in xs:
        _check_input(t, xs[0].device, xs[0].dtype)
    key = (tuple(tuple(t.shape) for t in xs), multi, xs[0].dtype, str(xs[0].device), ydbl_env())
    cache = m.__dict__.setdefault("_fwd_plans", {})
    mp = cache.pop(key, None)
    if mp is None:
        while len(cache) >= 2:
            cache.pop(next(iter(cache)))
        with torch.cuda.device(xs[0].device):
            mp = _ModulePlan(m, xs, multi)
    cache[key] = mp
    y = mp(xs)
    if weights_signature(m) != mp.wsig:  # weights edited since the plan folded them: rebuild, run again
        with torch.cuda.device(xs[0].device):
            mp = cache[key] = _ModulePlan(m, xs, multi)
        y = mp(xs)
    return y


class PlanModule(nn.Module):
    """Base of the built-in modules: ``forward(x)`` = run_module (the reference's ``m(x)`` contract)."""

    def forward(self, x):
        return run_module(self, x)


def _meta_copy(m: nn.Module) -> nn.Module:
    return copy.deepcopy(m).to("meta")


def torch_out_shape(m: nn.Module, src) -> tuple:
    """NHWC shape of a forward-only plugin's output, from a shape-only (meta) run of its forward on NCHW inputs
    of the given NHWC shapes."""
    multi = isinstance(src, list)
    metas = [torch.empty((s[0], s[3], s[1], s[2]), device="meta") for s in (src if multi else [src])]
    with torch.no_grad():
        y = _meta_copy(m)(metas if multi else metas[0])
    if not isinstance(y, torch.Tensor) or y.ndim != 4:
        raise TypeError(f"plugin {type(m).__name__}: forward must return one BCHW tensor")
    return (y.shape[0], y.shape[2], y.shape[3], y.shape[1])


def emit_torch(m: nn.Module, plan: Plan, x, out: TV | None = None) -> TV:
    """A registered plugin module that has only a torch ``forward`` (the reference's plugin contract: any class
    with forward(x), looked up by name, U/nn/tasks.py:974, called as m(x), :158-161) as one plan step: a device
    copy of the module in the plan's dtype (weights frozen at build, like every other layer) runs on NCHW views
    of its NHWC input slices, on the stream the plan runs on -- so it is captured into the step's hipGraph with
    the HIP launches around it -- and its result is copied into the output view.  The module's forward must be
    graph-capturable (no host syncs) and must launch on the current stream only (single_stream)."""
    multi = isinstance(x, (list, tuple))
    xs = list(x) if multi else [x]
    shape = torch_out_shape(m, [v.shape for v in xs] if multi else xs[0].shape)
    y = out if out is not None else plan.alloc(*shape)
    if y.shape != shape:
        raise ValueError(f"plugin {type(m).__name__}: output {shape} does not fit the destination {y.shape}")
    dm = copy.deepcopy(m).to(plan.device)
    if plan.device.type != "meta":
        dm = dm.to(plan.dtype)
    dm.eval()

    def step(stream):
        # handle 0 (c_void_p value None) is the null stream: eager runs on torch's default stream pass it
        ts = (torch.cuda.ExternalStream(stream.value, device=plan.device) if stream.value
              else torch.cuda.default_stream(plan.device))
        with torch.cuda.stream(ts), torch.no_grad():
            ins = [v.nchw() for v in xs]
            y.nchw().copy_(dm(ins if multi else ins[0]))
        return 0

    step.single_stream = True
    step.__name__ = f"torch:{type(m).__name__}"
    plan.steps.append(Step(step, (), f"torch.{type(m).__name__}", [dm]))
    return y


# =============================================================================== conv.py
class Conv(PlanModule):
    """U/nn/modules/conv.py:39-63 — conv -> BN -> SiLU (BN folded at plan time, as fuse() does)."""

    default_act = nn.SiLU()

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, d=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p, d), groups=g, dilation=d, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = self.default_act if act is True else act if isinstance(act, nn.Module) else nn.Identity()

    def folded(self):
        if hasattr(self, "bn"):
            return fold_bn(self.conv.weight, self.conv.bias, self.bn)
        return self.conv.weight.detach().float().cpu(), (
            self.conv.bias.detach().float().cpu() if self.conv.bias is not None else None)

    def emit(self, plan, x, out=None, res=None, res_mode=_lib.RES_NONE):
        w, b = self.folded()
        return emit_conv2d(plan, self.conv, x, out, w, b, _act_code(self.act), res, res_mode,
                           what=f"Conv{self.conv.kernel_size[0]}x{self.conv.kernel_size[0]}")


class DWConv(Conv):
    """U/nn/modules/conv.py:128-133."""

    def __init__(self, c1, c2, k=1, s=1, d=1, act=True):
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), d=d, act=act)


class DSConv(PlanModule):
    """U/nn/modules/conv.py:91-108 — dw -> pw -> BN -> SiLU."""

    def __init__(self, c_in, c_out, k=3, s=1, p=None, d=1, bias=False):
        super().__init__()
        if p is None:
            p = (d * (k - 1)) // 2
        self.dw = nn.Conv2d(c_in, c_in, kernel_size=k, stride=s, padding=p, dilation=d, groups=c_in, bias=bias)
        self.pw = nn.Conv2d(c_in, c_out, 1, 1, 0, bias=bias)
        self.bn = nn.BatchNorm2d(c_out)
        self.act = nn.SiLU()

    def emit(self, plan, x, out=None, res=None, res_mode=_lib.RES_NONE):
        w, b = fold_bn(self.pw.weight, self.pw.bias, self.bn)
        if self.dw.bias is None and fused_dsconv_ok(self.dw, x, plan.dtype):
            return emit_dsconv(plan, self.dw, x, out, w, b, _lib.ACT_SILU, res, res_mode)
        t = emit_conv2d(plan, self.dw, x, None, what=f"DSConv.dw{self.dw.kernel_size[0]}")
        return emit_conv2d(plan, self.pw, t, out, w, b, _lib.ACT_SILU, res, res_mode, what="DSConv.pw")


class GhostConv(PlanModule):
    """U/nn/modules/conv.py:184-197 — cat(y, dw5x5(y)), y = cv1(x)."""

    def __init__(self, c1, c2, k=1, s=1, g=1, act=True):
        super().__init__()
        c_ = c2 // 2
        self.cv1 = Conv(c1, c_, k, s, None, g, act=act)
        self.cv2 = Conv(c_, c_, 5, 1, None, c_, act=act)

    def emit(self, plan, x, out=None, res=None):
        c_ = self.cv1.conv.out_channels
        ho, wo = conv_out_hw(x.h, x.w, self.cv1.conv.kernel_size[0], self.cv1.conv.stride[0],
                             self.cv1.conv.padding[0], 1)
        y = out if out is not None else plan.alloc(x.n, ho, wo, 2 * c_)
        r0 = res.cslice(0, c_) if res is not None else None
        r1 = res.cslice(c_, c_) if res is not None else None
        # the dw half reads the pre-residual cv1 output, so with a residual cv1 goes to a temporary
        y0 = plan.alloc(x.n, ho, wo, c_) if res is not None else y.cslice(0, c_)
        self.cv1.emit(plan, x, y0)
        self.cv2.emit(plan, y0, y.cslice(c_, c_), res=r1, res_mode=_lib.RES_ADD if res is not None else 0)
        if res is not None:
            plan.launch("ydbl_gate_add", r0.struct(), y0.struct(), 1.0, y.cslice(0, c_).struct(), what="ghost.res")
        return y


class Concat(PlanModule):
    """U/nn/modules/conv.py:349-359 — inputs are normally already slices of the output (see tasks.py)."""

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension

    def emit(self, plan, xs, out=None):
        c = sum(x.c for x in xs)
        y = out if out is not None else plan.alloc(xs[0].n, xs[0].h, xs[0].w, c)
        off = 0
        for x in xs:
            dst = y.cslice(off, x.c)
            if not (x.base is dst.base and x.off == dst.off and x.cs == dst.cs):
                emit_copy(plan, x, dst)
            off += x.c
        return y


# =============================================================================== block.py
def emit_conv3x3_pair(plan, a: "Conv", b: "Conv", x: TV, out: TV | None = None) -> TV:
    """Conv(c, cm, 3) -> Conv(cm, c, 3) (SiLU both, no shortcut) as one ydbl_bottleneck_nhwc launch with
    the intermediate in LDS when the (c, cm) pair is built (fp16; used for the Detect box branch
    cv2[i][0:2] at 64 channels, head.py:86-90), else the two convs."""
    ca, cb = a.conv, b.conv
    c, cm = cb.out_channels, ca.out_channels
    ok = (plan.dtype == torch.float16 and not os.environ.get("YDBL_NO_BNECK") and not os.environ.get("YDBL_NO_PAIR3")
          and (c, cm) == (64, 64)
          and x.c == c == ca.in_channels and cb.in_channels == cm
          and all(m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1)
                  and m.groups == 1 for m in (ca, cb))
          and isinstance(a.act, nn.SiLU) and isinstance(b.act, nn.SiLU))
    y = out if out is not None else plan.alloc(x.n, x.h, x.w, c)
    if not ok or y.base is x.base:
        return b.emit(plan, a.emit(plan, x), out)
    args = [t.float().contiguous() for t in (*a.folded(), *b.folded())]
    host = torch.empty(int(_lib.lib.ydbl_conv3x3_pair_params_size(c, cm)), dtype=torch.uint8)
    _lib.check(_lib.lib.ydbl_conv3x3_pair_pack(*[t.data_ptr() for t in args], c, cm, host.data_ptr()),
               "ydbl_conv3x3_pair_pack")
    params = plan.const(host)
    d = _lib.BottleneckDesc(x.struct(), y.struct(), c, 0, 0, params.data_ptr(), cm)
    plan.launch("ydbl_bottleneck_nhwc", d, what=f"Conv3x3x2.c{c}", keep=[params, d])
    return y


def emit_detect_box(plan, seq, x: TV, out: TV) -> bool:
    """Detect box branch cv2[i] = Conv(c_in,64,3) -> Conv(64,64,3) -> Conv2d(64,64,1,bias) (head.py:86-90) as
    one ydbl_bottleneck_nhwc launch (desc.pw = 1: both 3x3 intermediates stay in LDS).  False (nothing
    emitted) unless fp16 with c_in 64 or 128 (DBL-n P3 / P4)."""
    a, b, c = seq[0], seq[1], seq[2]
    ca, cb = a.conv, b.conv
    ok = (plan.dtype == torch.float16 and not os.environ.get("YDBL_NO_BNECK") and not os.environ.get("YDBL_NO_BOX3")
          and x.c in (64, 128)
          and ca.in_channels == x.c and ca.out_channels == cb.in_channels == cb.out_channels == 64
          and all(m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1)
                  and m.groups == 1 for m in (ca, cb))
          and isinstance(a.act, nn.SiLU) and isinstance(b.act, nn.SiLU)
          and isinstance(c, nn.Conv2d) and c.kernel_size == (1, 1) and c.groups == 1 and c.bias is not None
          and c.in_channels == c.out_channels == 64 and out.c == 64 and out.base is not x.base)
    if not ok:
        return False
    args = [t.float().contiguous() for t in (*a.folded(), *b.folded())]
    args += [c.weight.detach().float().reshape(64, 64).contiguous(), c.bias.detach().float().contiguous()]
    host = torch.empty(int(_lib.lib.ydbl_detect_box_params_size(x.c, 64)), dtype=torch.uint8)
    _lib.check(_lib.lib.ydbl_detect_box_pack(*[t.data_ptr() for t in args], x.c, 64, host.data_ptr()),
               "ydbl_detect_box_pack")
    params = plan.const(host)
    d = _lib.BottleneckDesc(x.struct(), out.struct(), 64, 0, 0, params.data_ptr(), 64, 1)
    plan.launch("ydbl_bottleneck_nhwc", d, what="Detect.box3", keep=[params, d])
    return True


class Bottleneck(PlanModule):
    """U/nn/modules/block.py:344-357."""

    def __init__(self, c1, c2, shortcut=True, g=1, k=(3, 3), e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, k[0], 1)
        self.cv2 = Conv(c_, c2, k[1], 1, g=g)
        self.add = shortcut and c1 == c2

    def fused_ok(self, plan, x) -> bool:
        """cv1 -> cv2 as one ydbl_bottleneck_nhwc launch: fp16, c -> c/2 -> c, 3x3 s1 both, SiLU both."""
        a, b = self.cv1.conv, self.cv2.conv
        c = b.out_channels
        return (plan.dtype == torch.float16 and not os.environ.get("YDBL_NO_BNECK") and c in (16, 32, 64)
                and x.c == c == a.in_channels and a.out_channels == c // 2 == b.in_channels
                and all(m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1)
                        and m.dilation == (1, 1) and m.groups == 1 for m in (a, b))
                and isinstance(self.cv1.act, nn.SiLU) and isinstance(self.cv2.act, nn.SiLU))

    def emit(self, plan, x, out=None):
        if self.fused_ok(plan, x):
            c = x.c
            y = out if out is not None else plan.alloc(x.n, x.h, x.w, c)
            if y.base is not x.base:  # the kernel reads a halo of x while writing y
                args = [t.float().contiguous() for t in (*self.cv1.folded(), *self.cv2.folded())]
                host = torch.empty(int(_lib.lib.ydbl_bottleneck_params_size(c)), dtype=torch.uint8)
                _lib.check(_lib.lib.ydbl_bottleneck_pack(*[t.data_ptr() for t in args], c, host.data_ptr()),
                           "ydbl_bottleneck_pack")
                params = plan.const(host)
                d = _lib.BottleneckDesc(x.struct(), y.struct(), c, int(self.add), 0, params.data_ptr())
                plan.launch("ydbl_bottleneck_nhwc", d, what=f"Bottleneck.c{c}", keep=[params, d])
                return y
        t = self.cv1.emit(plan, x)
        return self.cv2.emit(plan, t, out, res=x if self.add else None,
                             res_mode=_lib.RES_ADD if self.add else _lib.RES_NONE)


class C2f(PlanModule):
    """U/nn/modules/block.py:234-249."""

    def __init__(self, c1, c2, n=1, shortcut=False, g=1, e=0.5):
        super().__init__()
        self.c = int(c2 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv((2 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(Bottleneck(self.c, self.c, shortcut, g, k=((3, 3), (3, 3)), e=1.0) for _ in range(n))

    def emit(self, plan, x, out=None):
        c, n = self.c, len(self.m)
        buf = plan.alloc(x.n, x.h, x.w, (2 + n) * c)
        self.cv1.emit(plan, x, buf.cslice(0, 2 * c))
        for i, m in enumerate(self.m):
            m.emit(plan, buf.cslice((1 + i) * c, c), buf.cslice((2 + i) * c, c))
        return self.cv2.emit(plan, buf, out)


class C3(PlanModule):
    """U/nn/modules/block.py:259-273."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=((1, 1), (3, 3)), e=1.0) for _ in range(n)))

    def emit(self, plan, x, out=None):
        c_ = self.cv1.conv.out_channels
        if mergeable([self.cv2, self.cv1]) and not os.environ.get("YDBL_NO_MERGE"):
            # cv2 and cv1 both read x: one launch into [m slot | cv2 | cv1] (cv3 reads the first 2c_)
            buf = plan.alloc(x.n, x.h, x.w, 3 * c_)
            emit_merged(plan, [self.cv2, self.cv1], x, buf.cslice(c_, 2 * c_))
            emit_seq(plan, self.m, buf.cslice(2 * c_, c_), buf.cslice(0, c_))
            return self.cv3.emit(plan, buf.cslice(0, 2 * c_), out)
        buf = plan.alloc(x.n, x.h, x.w, 2 * c_)
        t = self.cv1.emit(plan, x)
        emit_seq(plan, self.m, t, buf.cslice(0, c_))
        self.cv2.emit(plan, x, buf.cslice(c_, c_))
        return self.cv3.emit(plan, buf, out)


class GhostBottleneck(PlanModule):
    """U/nn/modules/block.py:323-341 (stride 1 on the DBL path)."""

    def __init__(self, c1, c2, k=3, s=1):
        super().__init__()
        c_ = c2 // 2
        self.conv = nn.Sequential(
            GhostConv(c1, c_, 1, 1),
            DWConv(c_, c_, k, s, act=False) if s == 2 else nn.Identity(),
            GhostConv(c_, c2, 1, 1, act=False),
        )
        self.shortcut = (
            nn.Sequential(DWConv(c1, c1, k, s, act=False), Conv(c1, c2, 1, 1, act=False)) if s == 2 else nn.Identity()
        )

    def emit(self, plan, x, out=None):
        if not isinstance(self.shortcut, nn.Identity):
            raise NotImplementedError("GhostBottleneck s=2 is not on the DBL path")
        t = self.conv[0].emit(plan, x)
        return self.conv[2].emit(plan, t, out, res=x)


class C3Ghost(C3):
    """U/nn/modules/block.py:313-320."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(GhostBottleneck(c_, c_) for _ in range(n)))


class DSBottleneck(PlanModule):
    """U/nn/modules/block.py:1408-1444."""

    def __init__(self, c1, c2, shortcut=True, e=0.5, k1=3, k2=5, d2=1):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = DSConv(c1, c_, k1, s=1, p=None, d=1)
        self.cv2 = DSConv(c_, c2, k2, s=1, p=None, d=d2)
        self.add = shortcut and c1 == c2

    def emit(self, plan, x, out=None):
        t = self.cv1.emit(plan, x)
        return self.cv2.emit(plan, t, out, res=x if self.add else None,
                             res_mode=_lib.RES_ADD if self.add else _lib.RES_NONE)


class DSC3k(C3):
    """U/nn/modules/block.py:1447-1503."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, k1=3, k2=5, d2=1):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(
            *(DSBottleneck(c_, c_, shortcut=shortcut, e=1.0, k1=k1, k2=k2, d2=d2) for _ in range(n))
        )


class DSC3k2(C2f):
    """U/nn/modules/block.py:1505-1580."""

    def __init__(self, c1, c2, n=1, dsc3k=False, e=0.5, g=1, shortcut=True, k1=3, k2=7, d2=1):
        super().__init__(c1, c2, n, shortcut, g, e)
        if dsc3k:
            self.m = nn.ModuleList(
                DSC3k(self.c, self.c, n=2, shortcut=shortcut, g=g, e=1.0, k1=k1, k2=k2, d2=d2) for _ in range(n)
            )
        else:
            self.m = nn.ModuleList(
                DSBottleneck(self.c, self.c, shortcut=shortcut, e=1.0, k1=k1, k2=k2, d2=d2) for _ in range(n)
            )


class SPPF(PlanModule):
    """U/nn/modules/block.py:179-198 — cv1 writes slice 0 of one [n,h,w,4c_] buffer, one ydbl_maxpool5_cascade launch
    fills slices 1-3 (the three chained 5x5 max-pools), cv2 reads the buffer: no concat copy."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)

    def emit(self, plan, x, out=None):
        if self.m.kernel_size != 5:
            raise NotImplementedError(f"SPPF: k={self.m.kernel_size}; the HIP pool cascade is built for 5")
        c_ = self.cv1.conv.out_channels
        buf = plan.alloc(x.n, x.h, x.w, 4 * c_)
        self.cv1.emit(plan, x, buf.cslice(0, c_))
        d = _lib.MaxPool5Desc(*[buf.cslice(i * c_, c_).struct() for i in range(4)], 5)
        plan.launch("ydbl_maxpool5_cascade", d, what="SPPF.pool5x3", keep=[d])
        return self.cv2.emit(plan, buf, out)


class C3k(C3):
    """U/nn/modules/block.py:745-753 — C3 with k x k Bottlenecks at e=1.0."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, k=3):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(Bottleneck(c_, c_, shortcut, g, k=(k, k), e=1.0) for _ in range(n)))


class C3k2(C2f):
    """U/nn/modules/block.py:734-742 — C2f whose blocks are C3k(c, c, 2) or the default Bottleneck (k=(3, 3), e=0.5,
    unlike C2f's own); they chain through the slices of the concat buffer (C2f.emit)."""

    def __init__(self, c1, c2, n=1, c3k=False, e=0.5, g=1, shortcut=True):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(
            C3k(self.c, self.c, 2, shortcut, g) if c3k else Bottleneck(self.c, self.c, shortcut, g) for _ in range(n))


class Attention(PlanModule):
    """U/nn/modules/block.py:896-930 — qkv 1x1 -> softmax(q^T k / sqrt(key_dim)) v over all tokens (ydbl_psa_attn)
    -> + pe(v) (3x3 depthwise, the add in its epilogue) -> proj 1x1."""

    def __init__(self, dim, num_heads=8, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim**-0.5
        nh_kd = self.key_dim * num_heads
        h = dim + nh_kd * 2
        self.qkv = Conv(dim, h, 1, act=False)
        self.proj = Conv(dim, dim, 1, act=False)
        self.pe = Conv(dim, dim, 3, 1, g=dim, act=False)

    def emit(self, plan, x, out=None, res=None):
        """res: a view added to the result in proj's epilogue (PSABlock's x + attn(x))."""
        if self.head_dim != 64 or self.key_dim != 32:
            raise NotImplementedError(f"Attention: head_dim {self.head_dim}, key_dim {self.key_dim}; the HIP kernel "
                                      "is built for 64 / 32 (C2PSA's)")
        c = self.num_heads * self.head_dim
        qkv = self.qkv.emit(plan, x)
        att, v = plan.alloc(x.n, x.h, x.w, c), plan.alloc(x.n, x.h, x.w, c)
        d = _lib.PsaAttnDesc(qkv.struct(), att.struct(), v.struct(), self.num_heads, self.key_dim, self.head_dim,
                             self.scale)
        plan.launch("ydbl_psa_attn", d, what="PSA.attn", keep=[d])
        t = self.pe.emit(plan, v, None, res=att, res_mode=_lib.RES_ADD)  # attention + pe(v)
        return self.proj.emit(plan, t, out, res=res, res_mode=_lib.RES_ADD if res is not None else _lib.RES_NONE)


class PSABlock(PlanModule):
    """U/nn/modules/block.py:955-967 — x + attn(x), then x + ffn(x); both adds ride in conv epilogues."""

    def __init__(self, c, attn_ratio=0.5, num_heads=4, shortcut=True):
        super().__init__()
        self.attn = Attention(c, attn_ratio=attn_ratio, num_heads=num_heads)
        self.ffn = nn.Sequential(Conv(c, c * 2, 1), Conv(c * 2, c, 1, act=False))
        self.add = shortcut

    def emit(self, plan, x, out=None):
        """out may be x itself (C2PSA's last block): the launches that read x (qkv, proj's residual) precede
        ffn[1], which reads only buffers of this block."""
        x1 = self.attn.emit(plan, x, None, res=x if self.add else None)
        h = self.ffn[0].emit(plan, x1)
        return self.ffn[1].emit(plan, h, out, res=x1 if self.add else None,
                                res_mode=_lib.RES_ADD if self.add else _lib.RES_NONE)


class C2PSA(PlanModule):
    """U/nn/modules/block.py:1038-1052 — cv1 writes [a | b] into one 2c buffer, the n PSABlocks run b -> b', the last
    one back into the b slice, cv2 reads the buffer."""

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.m = nn.Sequential(*(PSABlock(self.c, attn_ratio=0.5, num_heads=self.c // 64) for _ in range(n)))

    def emit(self, plan, x, out=None):
        c, n = self.c, len(self.m)
        buf = plan.alloc(x.n, x.h, x.w, 2 * c)
        self.cv1.emit(plan, x, buf)
        b = buf.cslice(c, c)
        for i, m in enumerate(self.m):  # intermediate b's get buffers of their own
            b = m.emit(plan, b, buf.cslice(c, c) if i == n - 1 else None)
        return self.cv2.emit(plan, buf, out)


class PSA(PlanModule):
    """U/nn/modules/block.py:970-1010 (YOLOv10) — C2PSA's body for one block, written out: cv1 writes [a | b] into one
    2c buffer, b + attn(b) and b + ffn(b) ride in proj's and ffn[1]'s epilogues, the last one back into the b slice,
    cv2 reads the buffer.  num_heads = c // 64, so every stock scale meets Attention's head_dim 64 / key_dim 32."""

    def __init__(self, c1, c2, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.attn = Attention(self.c, attn_ratio=0.5, num_heads=self.c // 64)
        self.ffn = nn.Sequential(Conv(self.c, self.c * 2, 1), Conv(self.c * 2, self.c, 1, act=False))

    def emit(self, plan, x, out=None):
        c = self.c
        buf = plan.alloc(x.n, x.h, x.w, 2 * c)
        self.cv1.emit(plan, x, buf)
        b = buf.cslice(c, c)
        b1 = self.attn.emit(plan, b, None, res=b)
        h = self.ffn[0].emit(plan, b1)
        self.ffn[1].emit(plan, h, b, res=b1, res_mode=_lib.RES_ADD)  # (b's readers, qkv and proj, are behind us)
        return self.cv2.emit(plan, buf, out)


class SCDown(PlanModule):
    """U/nn/modules/block.py:1088-1120 (YOLOv10) — Conv 1x1, then a depthwise k x k stride-s Conv without activation."""

    def __init__(self, c1, c2, k, s):
        super().__init__()
        self.cv1 = Conv(c1, c2, 1, 1)
        self.cv2 = Conv(c2, c2, k=k, s=s, g=c2, act=False)

    def emit(self, plan, x, out=None):
        return self.cv2.emit(plan, self.cv1.emit(plan, x), out)


@torch.no_grad()
def _fuse_conv_bn(conv: nn.Conv2d, bn: nn.BatchNorm2d) -> nn.Conv2d:
    """fuse_conv_and_bn (U/utils/torch_utils.py:238-265), its op sequence, as a new nn.Conv2d with a bias."""
    fused = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                      conv.dilation, conv.groups, bias=True).requires_grad_(False).to(conv.weight.device)
    w_conv = conv.weight.view(conv.out_channels, -1)
    w_bn = torch.diag(bn.weight.div(torch.sqrt(bn.eps + bn.running_var)))
    fused.weight.copy_(torch.mm(w_bn, w_conv).view(fused.weight.shape))
    b_conv = (torch.zeros(conv.weight.shape[0], device=conv.weight.device, dtype=conv.weight.dtype)
              if conv.bias is None else conv.bias)
    b_bn = bn.bias - bn.weight.mul(bn.running_mean).div(torch.sqrt(bn.running_var + bn.eps))
    fused.bias.copy_(torch.mm(w_bn, b_conv.reshape(-1, 1)).reshape(-1) + b_bn)
    return fused


class RepVGGDW(PlanModule):
    """U/nn/modules/block.py:756-815 (YOLOv10) — SiLU(dw7x7(x) + dw3x3(x)), both with BN, as ONE 7x7 depthwise launch:
    the weights are folded when the plan is built exactly as fuse() folds them (BN into both, the 3x3 zero-padded to
    7x7, weights and biases added).  fuse() -- the reference's, called by DetectionModel.fuse() -- leaves ``conv`` an
    nn.Conv2d with a bias and no ``conv1``; both forms are accepted, and both load their own state_dict."""

    def __init__(self, ed):
        super().__init__()
        self.conv = Conv(ed, ed, 7, 1, 3, g=ed, act=False)
        self.conv1 = Conv(ed, ed, 3, 1, 1, g=ed, act=False)
        self.dim = ed
        self.act = nn.SiLU()

    @property
    def conv2d(self) -> nn.Conv2d:
        """The 7x7 depthwise nn.Conv2d (its geometry is the launch's), fused or not."""
        return self.conv.conv if isinstance(self.conv, Conv) else self.conv

    @torch.no_grad()
    def fuse(self):
        """block.py:791-815."""
        if not hasattr(self, "conv1"):
            return
        conv = _fuse_conv_bn(self.conv.conv, self.conv.bn)
        conv1 = _fuse_conv_bn(self.conv1.conv, self.conv1.bn)
        conv1_w = torch.nn.functional.pad(conv1.weight, [2, 2, 2, 2])
        final_w, final_b = conv.weight + conv1_w, conv.bias + conv1.bias
        conv.weight.data.copy_(final_w)
        conv.bias.data.copy_(final_b)
        self.conv = conv
        del self.conv1

    def folded(self):
        """(w [c, 1, 7, 7], b [c]) fp32 on the host: fuse()'s arithmetic, the module left as it is."""
        if not hasattr(self, "conv1"):
            return self.conv.weight.detach().float().cpu(), self.conv.bias.detach().float().cpu()
        (w7, b7), (w3, b3) = self.conv.folded(), self.conv1.folded()
        return w7 + torch.nn.functional.pad(w3, [2, 2, 2, 2]), b7 + b3

    def emit(self, plan, x, out=None, res=None, res_mode=_lib.RES_NONE):
        w, b = self.folded()
        return emit_conv2d(plan, self.conv2d, x, out, w, b, _act_code(self.act), res, res_mode, what="RepVGGDW.dw7")


class _RepDW:
    """What emit_dw_pw reads of a DWConv (conv, act, folded, emit), for a RepVGGDW."""

    def __init__(self, m: RepVGGDW):
        self.conv, self.act, self.folded, self.emit = m.conv2d, m.act, m.folded, m.emit


class CIB(PlanModule):
    """U/nn/modules/block.py:818-850 (YOLOv10) — dw3 -> pw -> dw3 (lk: RepVGGDW) -> pw -> dw3 [+ x].  The two
    depthwise -> pointwise pairs go through emit_dw_pw (one launch each where the fused DSConv kernel takes the
    shape, else two); the shortcut rides in the last depthwise conv's epilogue."""

    def __init__(self, c1, c2, shortcut=True, e=0.5, lk=False):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = nn.Sequential(
            Conv(c1, c1, 3, g=c1),
            Conv(c1, 2 * c_, 1),
            RepVGGDW(2 * c_) if lk else Conv(2 * c_, 2 * c_, 3, g=2 * c_),
            Conv(2 * c_, c2, 1),
            Conv(c2, c2, 3, g=c2),
        )
        self.add = shortcut and c1 == c2

    def emit(self, plan, x, out=None):
        m = self.cv1
        t, _ = emit_dw_pw(plan, m[0], m[1], x, what="CIB.dw+pw")
        dw = _RepDW(m[2]) if isinstance(m[2], RepVGGDW) else m[2]
        t, _ = emit_dw_pw(plan, dw, m[3], t, what="CIB.dw+pw")
        return m[4].emit(plan, t, out, res=x if self.add else None,
                         res_mode=_lib.RES_ADD if self.add else _lib.RES_NONE)


class C2fCIB(C2f):
    """U/nn/modules/block.py:853-880 (YOLOv10) — C2f whose blocks are CIBs; they chain through the slices of the concat
    buffer (C2f.emit)."""

    def __init__(self, c1, c2, n=1, shortcut=False, lk=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(CIB(self.c, self.c, shortcut, e=1.0, lk=lk) for _ in range(n))


class AAttn(PlanModule):
    """U/nn/modules/block.py:1187-1264 — area attention: qkv 1x1 -> softmax(q^T k / sqrt(d)) v inside each of the
    `area` contiguous token chunks (ydbl_area_attn) -> + pe(v) (7x7 depthwise) -> proj 1x1."""

    def __init__(self, dim, num_heads, area=1):
        super().__init__()
        self.area = area
        self.num_heads = num_heads
        self.head_dim = head_dim = dim // num_heads
        all_head_dim = head_dim * self.num_heads
        self.qkv = Conv(dim, all_head_dim * 3, 1, act=False)
        self.proj = Conv(all_head_dim, dim, 1, act=False)
        self.pe = Conv(all_head_dim, dim, 7, 1, 3, g=dim, act=False)

    def emit(self, plan, x, out=None, res=None):
        """res: a view added to the result in proj's epilogue (ABlock's x + attn(x))."""
        if self.head_dim != 32:
            raise NotImplementedError(f"AAttn: head_dim {self.head_dim}; the HIP kernel is built for 32 (A2C2f's)")
        if (x.h * x.w) % self.area:
            raise ValueError(f"AAttn: {x.h}x{x.w} tokens do not split into {self.area} areas")
        c = self.num_heads * self.head_dim
        qkv = self.qkv.emit(plan, x)
        att, v = plan.alloc(x.n, x.h, x.w, c), plan.alloc(x.n, x.h, x.w, c)
        d = _lib.AreaAttnDesc(qkv.struct(), att.struct(), v.struct(), self.num_heads, self.area, self.head_dim**-0.5)
        plan.launch("ydbl_area_attn", d, what=f"AAttn.area{self.area}", keep=[d])
        t = self.pe.emit(plan, v, None, res=att, res_mode=_lib.RES_ADD)  # x + pe(v)
        return self.proj.emit(plan, t, out, res=res, res_mode=_lib.RES_ADD if res is not None else _lib.RES_NONE)


class ABlock(PlanModule):
    """U/nn/modules/block.py:1268-1322 — x + attn(x), then x + mlp(x); both adds ride in conv epilogues."""

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

    def emit(self, plan, x, out=None):
        x1 = self.attn.emit(plan, x, None, res=x)
        (w0, b0), (w1, b1) = self.mlp[0].folded(), self.mlp[1].folded()
        hid = w0.shape[0]
        pad = round_up(hid, 8) - hid  # int(dim * mlp_ratio) need not be whole channel vectors (128 * 1.2 = 153):
        if pad:  # zero output rows make the pad channels SiLU(0) = 0, and mlp[1]'s K is zero-padded to match
            w0 = torch.nn.functional.pad(w0, (0, 0, 0, 0, 0, 0, 0, pad))
            b0 = torch.nn.functional.pad(b0 if b0 is not None else torch.zeros(hid), (0, pad))
        h = plan.alloc(x.n, x.h, x.w, hid + pad)
        emit_dense(plan, x1, h, w0, b0, act=_act_code(self.mlp[0].act), what="Conv1x1")
        y = out if out is not None else plan.alloc(x.n, x.h, x.w, x.c)
        emit_dense(plan, h, y, w1, b1, act=_act_code(self.mlp[1].act), res=x1, res_mode=_lib.RES_ADD, what="Conv1x1")
        return y


class A2C2f(PlanModule):
    """U/nn/modules/block.py:1325-1406 — cv1, n x (ABlock, ABlock) chained through the slices of one concat buffer,
    cv2; residual=True: x + gamma[c] * y (ydbl_channel_gate_add: cv2 has a SiLU, gamma does not fold into it)."""

    def __init__(self, c1, c2, n=1, a2=True, area=1, residual=False, mlp_ratio=2.0, e=0.5, g=1, shortcut=True):
        super().__init__()
        c_ = int(c2 * e)
        assert c_ % 32 == 0, "Dimension of ABlock must be a multiple of 32."
        if not a2:
            raise NotImplementedError("A2C2f(a2=False), the C3k form, has no HIP path (no v13 config uses it)")
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv((1 + n) * c_, c2, 1)
        self.gamma = nn.Parameter(0.01 * torch.ones(c2), requires_grad=True) if a2 and residual else None
        self.m = nn.ModuleList(
            nn.Sequential(*(ABlock(c_, c_ // 32, mlp_ratio, area) for _ in range(2))) for _ in range(n))

    def emit(self, plan, x, out=None):
        c_, n = self.cv1.conv.out_channels, len(self.m)
        buf = plan.alloc(x.n, x.h, x.w, (1 + n) * c_)
        self.cv1.emit(plan, x, buf.cslice(0, c_))
        for i, m in enumerate(self.m):
            emit_seq(plan, m, buf.cslice(i * c_, c_), buf.cslice((i + 1) * c_, c_))
        if self.gamma is None:
            return self.cv2.emit(plan, buf, out)
        t = self.cv2.emit(plan, buf)
        y = out if out is not None else plan.alloc(x.n, x.h, x.w, t.c)
        g = plan.const(self.gamma.detach().float())
        plan.launch("ydbl_channel_gate_add", x.struct(), t.struct(), g.data_ptr(), y.struct(), what="A2C2f.gamma",
                    keep=[g])
        return y


class Upsample(PlanModule):
    """nn.Upsample(size, scale_factor, mode) as a YAML layer ('nn.Upsample', [None, 2, "nearest"]): nearest x2 only,
    ydbl_pool_up_concat's third segment."""

    def __init__(self, size=None, scale_factor=None, mode="nearest"):
        super().__init__()
        if size is not None or scale_factor is None or float(scale_factor) != 2.0 or mode != "nearest":
            raise NotImplementedError(f"Upsample(size={size}, scale_factor={scale_factor}, mode={mode!r}): only "
                                      "scale_factor=2, mode='nearest' has a HIP path")
        self.size, self.scale_factor, self.mode = size, scale_factor, mode

    def forward(self, x):
        if isinstance(x, torch.Tensor) and x.device.type in ("cpu", "meta"):
            return nn.functional.interpolate(x, None, float(self.scale_factor), self.mode)
        return run_module(self, x)

    def emit(self, plan, x, out=None):
        y = out if out is not None else plan.alloc(x.n, 2 * x.h, 2 * x.w, x.c)
        plan.launch("ydbl_pool_up_concat", None, None, x.struct(), y.struct(), what="Upsample.nearest2")
        return y


class AdaHyperedgeGen(nn.Module):
    """U/nn/modules/block.py:1582-1657 (parameters only; compute in ydbl_hg_*)."""

    def __init__(self, node_dim, num_hyperedges, num_heads=4, dropout=0.1, context="both"):
        super().__init__()
        if context != "both":
            raise NotImplementedError("only context='both' (the DBL configuration) has a HIP path")
        self.num_heads = num_heads
        self.num_hyperedges = num_hyperedges
        self.head_dim = node_dim // num_heads
        self.context = context
        self.prototype_base = nn.Parameter(torch.Tensor(num_hyperedges, node_dim))
        nn.init.xavier_uniform_(self.prototype_base)
        self.context_net = nn.Linear(2 * node_dim, num_hyperedges * node_dim)
        self.pre_head_proj = nn.Linear(node_dim, node_dim)
        self.dropout = nn.Dropout(dropout)
        self.scaling = math.sqrt(self.head_dim)


class AdaHGConv(PlanModule):
    """U/nn/modules/block.py:1659-1708."""

    def __init__(self, embed_dim, num_hyperedges=16, num_heads=4, dropout=0.1, context="both"):
        super().__init__()
        self.edge_generator = AdaHyperedgeGen(embed_dim, num_hyperedges, num_heads, dropout, context)
        self.edge_proj = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.GELU())
        self.node_proj = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.GELU())

    def _params(self, plan):
        g, c = self.edge_generator, plan.const
        return [c(g.prototype_base.float()), c(g.context_net.weight.float()), c(g.context_net.bias.float()),
                c(self.edge_proj[0].weight.float()), c(self.edge_proj[0].bias.float()),
                c(self.node_proj[0].weight.float()), c(self.node_proj[0].bias.float())]

    def fused_desc(self, plan, x, y, p=None):
        """(HgDesc, keep-list) of the one-call route (ydbl_hg_fused / ydbl_hg_fused_pair), or None where the
        staged route has to run: YDBL_HG_UNFUSED, a head_dim other than 16, a (dim, edges, tokens) the fused
        kernels do not take, or y intersecting x."""
        g = self.edge_generator
        D, E = x.c, g.num_hyperedges
        nws = _lib.lib.ydbl_hg_fused_workspace(x.n, x.h * x.w, D, E, _lib.dtype_code(plan.dtype))
        if (os.environ.get("YDBL_HG_UNFUSED") or D != 16 * g.num_heads or nws <= 0
                or not (y.base is not x.base or y.off + y.c <= x.off or x.off + x.c <= y.off)):
            return None
        p = self._params(plan) if p is None else p
        c = plan.const
        pw = c(g.pre_head_proj.weight.detach().float().to(plan.dtype).contiguous())
        pb = c(g.pre_head_proj.bias.detach().float())
        ws = plan.scratch(nws)  # per-slice partials, fully written before they are read
        d = HgDesc(x.struct(), _null_view(), y.struct(), E, g.num_heads, *[t.data_ptr() for t in p], ws.data_ptr(),
                   pw.data_ptr(), pb.data_ptr())
        return d, [d, pw, pb, ws, *p]

    def emit(self, plan, x, out=None):
        g = self.edge_generator
        D, E = x.c, g.num_hyperedges
        y = out if out is not None else plan.alloc(x.n, x.h, x.w, D)
        p = self._params(plan)
        fused = self.fused_desc(plan, x, y, p)
        if fused is not None:
            # the whole AdaHGConv, pre_head_proj included, from one C-ABI call (csrc/hg_fused.hip: five kernels
            # over (token slice, image) and (hyperedge, image) workgroups)
            plan.launch("ydbl_hg_fused", fused[0], what="AdaHG.fused", keep=fused[1])
            return y
        # X_proj = pre_head_proj(X) as a 1x1 conv over the token grid
        xp = plan.alloc(x.n, x.h, x.w, D)
        emit_dense(plan, x, xp, g.pre_head_proj.weight.detach().float().cpu().view(D, D, 1, 1),
                   g.pre_head_proj.bias.detach().float().cpu(), what="AdaHG.pre_proj")
        ws = plan.scratch(_lib.lib.ydbl_hg_workspace(x.n, x.h * x.w, D, E))
        d = HgDesc(x.struct(), xp.struct(), y.struct(), E, g.num_heads, *[t.data_ptr() for t in p], ws.data_ptr())
        plan.launch("ydbl_hg_context", d, what="AdaHG.context", keep=[d, ws, *p])
        plan.launch("ydbl_hg_propagate", d, what="AdaHG.propagate", keep=[d])
        return y


class AdaHGComputation(PlanModule):
    """U/nn/modules/block.py:1710-1752 (NHWC pixels are already the token sequence)."""

    def __init__(self, embed_dim, num_hyperedges=16, num_heads=8, dropout=0.1, context="both"):
        super().__init__()
        self.embed_dim = embed_dim
        self.hgnn = AdaHGConv(embed_dim, num_hyperedges, num_heads, dropout, context)

    def emit(self, plan, x, out=None):
        return self.hgnn.emit(plan, x, out)


class C3AH(PlanModule):
    """U/nn/modules/block.py:1754-1795."""

    def __init__(self, c1, c2, e=1.0, num_hyperedges=8, context="both"):
        super().__init__()
        c_ = int(c2 * e)
        assert c_ % 16 == 0, "Dimension of AdaHGComputation should be a multiple of 16."
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.m = AdaHGComputation(c_, num_hyperedges, c_ // 16, 0.1, context)
        self.cv3 = Conv(2 * c_, c2, 1)

    def emit(self, plan, x, out=None):
        c_ = self.cv1.conv.out_channels
        if mergeable([self.cv2, self.cv1]) and not os.environ.get("YDBL_NO_MERGE"):
            buf = plan.alloc(x.n, x.h, x.w, 3 * c_)  # [m slot | cv2 | cv1], as C3.emit
            emit_merged(plan, [self.cv2, self.cv1], x, buf.cslice(c_, 2 * c_))
            self.m.emit(plan, buf.cslice(2 * c_, c_), buf.cslice(0, c_))
            return self.cv3.emit(plan, buf.cslice(0, 2 * c_), out)
        buf = plan.alloc(x.n, x.h, x.w, 2 * c_)
        t = self.cv1.emit(plan, x)
        self.m.emit(plan, t, buf.cslice(0, c_))
        self.cv2.emit(plan, x, buf.cslice(c_, c_))
        return self.cv3.emit(plan, buf, out)


class FuseModule(PlanModule):
    """U/nn/modules/block.py:1797-1840."""

    def __init__(self, c_in, channel_adjust):
        super().__init__()
        self.downsample = nn.AvgPool2d(kernel_size=2)
        self.upsample = nn.Upsample(scale_factor=2, mode="nearest")
        self.conv_out = Conv((4 if channel_adjust else 3) * c_in, c_in, 1)

    def emit(self, plan, xs, out=None):
        p3, p4, p5 = xs
        cat = plan.alloc(p4.n, p4.h, p4.w, p3.c + p4.c + p5.c)
        plan.launch("ydbl_pool_up_concat", p3.struct(), p4.struct(), p5.struct(), cat.struct(), what="Fuse.cat")
        return self.conv_out.emit(plan, cat, out)


class HyperACE(PlanModule):
    """U/nn/modules/block.py:1842-1895."""

    def __init__(self, c1, c2, n=1, num_hyperedges=8, dsc3k=True, shortcut=False, e1=0.5, e2=1, context="both",
                 channel_adjust=True):
        super().__init__()
        self.c = int(c2 * e1)
        self.cv1 = Conv(c1, 3 * self.c, 1, 1)
        self.cv2 = Conv((4 + n) * self.c, c2, 1)
        self.m = nn.ModuleList(
            DSC3k(self.c, self.c, 2, shortcut, k1=3, k2=7) if dsc3k else DSBottleneck(self.c, self.c, shortcut=shortcut)
            for _ in range(n)
        )
        self.fuse = FuseModule(c1, channel_adjust)
        self.branch1 = C3AH(self.c, self.c, e2, num_hyperedges, context)
        self.branch2 = C3AH(self.c, self.c, e2, num_hyperedges, context)

    def emit(self, plan, xs, out=None):
        c, n = self.c, len(self.m)
        x = self.fuse.emit(plan, xs)
        # concat order of the reference: [y0, branch1(y1), y2, m_0(y2), ..., m_{n-1}, branch2(y1)]
        cat = plan.alloc(x.n, x.h, x.w, (4 + n) * c)
        self.cv1.emit(plan, x, cat.cslice(0, 3 * c))  # y0 | y1 | y2
        y1 = cat.cslice(c, c)
        if self._branches_mergeable():
            self._emit_branches(plan, y1, cat.cslice(c, c), cat.cslice((3 + n) * c, c))
        else:
            self.branch2.emit(plan, y1, cat.cslice((3 + n) * c, c))
            self.branch1.emit(plan, y1, cat.cslice(c, c))  # reads y1 before its last conv overwrites it
        prev = cat.cslice(2 * c, c)
        for i, m in enumerate(self.m):
            prev = m.emit(plan, prev, cat.cslice((3 + i) * c, c))
        return self.cv2.emit(plan, cat, out)


    def _branches_mergeable(self) -> bool:
        b1, b2 = self.branch1, self.branch2
        return (not os.environ.get("YDBL_NO_MERGE") and mergeable([b2.cv2, b2.cv1, b1.cv1, b1.cv2])
                and b1.cv1.conv.out_channels == b2.cv1.conv.out_channels)

    def _emit_branches(self, plan, y1, out1, out2):
        """Both C3AH branches read y1 (block.py:1886-1895): their four input 1x1s (cv1, cv2 of each) run as ONE
        launch into one buffer laid out [b2.m | b2.cv2 | b2.cv1 | b1.cv1 | b1.cv2 | b1.m], so each branch's
        cv3 input is contiguous: b2's in the reference order cat(m, cv2), b1's as (cv2, m) with cv3's weight
        columns swapped to match (the same sums, in another order of K).  The two AdaHGConvs are independent
        (disjoint slices of bb), so where both take the one-call route they share its five launches
        (ydbl_hg_fused_pair); YDBL_NO_HG_PAIR=1 keeps a call per branch."""
        b1, b2 = self.branch1, self.branch2
        c_ = b1.cv1.conv.out_channels
        bb = plan.alloc(y1.n, y1.h, y1.w, 6 * c_)
        emit_merged(plan, [b2.cv2, b2.cv1, b1.cv1, b1.cv2], y1, bb.cslice(c_, 4 * c_), what="C3AHx2.cv1|cv2")
        x2, m2, x1, m1 = bb.cslice(2 * c_, c_), bb.cslice(0, c_), bb.cslice(3 * c_, c_), bb.cslice(5 * c_, c_)
        f2 = f1 = None
        if not os.environ.get("YDBL_NO_HG_PAIR"):
            f2 = b2.m.hgnn.fused_desc(plan, x2, m2)
            f1 = b1.m.hgnn.fused_desc(plan, x1, m1) if f2 is not None else None
        if f1 is not None:
            plan.launch("ydbl_hg_fused_pair", f2[0], f1[0], what="AdaHG.fused2", keep=[*f2[1], *f1[1]])
            b2.cv3.emit(plan, bb.cslice(0, 2 * c_), out2)
        else:
            b2.m.emit(plan, x2, m2)
            b2.cv3.emit(plan, bb.cslice(0, 2 * c_), out2)
            b1.m.emit(plan, x1, m1)
        w, b = b1.cv3.folded()
        w = torch.cat([w[:, c_:], w[:, :c_]], 1)
        emit_conv2d(plan, b1.cv3.conv, bb.cslice(4 * c_, 2 * c_), out1, w, b, _act_code(b1.cv3.act), what="Conv1x1")


class DownsampleConv(PlanModule):
    """U/nn/modules/block.py:1897-1928."""

    def __init__(self, in_channels, channel_adjust=True):
        super().__init__()
        self.downsample = nn.AvgPool2d(kernel_size=2)
        self.channel_adjust = Conv(in_channels, in_channels * 2, 1) if channel_adjust else nn.Identity()

    def emit(self, plan, x, out=None):
        adjust = not isinstance(self.channel_adjust, nn.Identity)
        pooled = out if (out is not None and not adjust) else plan.alloc(x.n, x.h // 2, x.w // 2, x.c)
        plan.launch("ydbl_pool_up_concat", x.struct(), None, None, pooled.struct(), what="Downsample.pool")
        return self.channel_adjust.emit(plan, pooled, out) if adjust else pooled


class FullPAD_Tunnel(PlanModule):  # noqa: N801 (reference name)
    """U/nn/modules/block.py:1930-1956 — x0 + gate * x1."""

    def __init__(self):
        super().__init__()
        self.gate = nn.Parameter(torch.tensor(0.0))

    def emit(self, plan, xs, out=None):
        a, b = xs
        y = out if out is not None else plan.alloc(a.n, a.h, a.w, a.c)
        g = float(self.gate.detach().float().cpu())
        # Fused into the dense conv that produced the later of the two inputs (its epilogue writes
        # y = a + g*b as a second output; the other input is complete by then).  Otherwise one
        # ydbl_gate_add launch.
        if os.environ.get("YDBL_NO_FUSE_PAD"):  # A/B switch for the benches
            return self._launch(plan, a, b, g, y)
        ia, ib = plan.writer_of(a), plan.writer_of(b)
        if ib is not None and (ia is None or ia[0] < ib[0]) and (ia is not None or plan.made_before(a, ib[0])):
            return plan.fuse_second_output(ib, y, a, g, 1.0) or self._launch(plan, a, b, g, y)
        if ia is not None and (ib is None or ib[0] < ia[0]) and (ib is not None or plan.made_before(b, ia[0])):
            return plan.fuse_second_output(ia, y, b, 1.0, g) or self._launch(plan, a, b, g, y)
        return self._launch(plan, a, b, g, y)

    @staticmethod
    def _launch(plan, a, b, g, y):
        plan.launch("ydbl_gate_add", a.struct(), b.struct(), g, y.struct(), what="FullPAD")
        return y


# =============================================================================== DySample / LSKblock
class DySample(PlanModule):
    """U/nn/modules_upsample/DySample.py:20-81 (style 'lp', scale 2, groups 4, no scope)."""

    def __init__(self, in_channels, scale=2, style="lp", groups=4, dyscope=False):
        super().__init__()
        if style != "lp" or dyscope or scale != 2:
            raise NotImplementedError("DySample: only style='lp', scale=2, dyscope=False has a HIP path")
        assert in_channels >= groups and in_channels % groups == 0
        self.scale, self.style, self.groups = scale, style, groups
        self.offset = nn.Conv2d(in_channels, 2 * groups * scale**2, 1)
        nn.init.normal_(self.offset.weight, 0, 0.001)
        nn.init.constant_(self.offset.bias, 0)
        self.register_buffer("init_pos", self._init_pos())

    def _init_pos(self):
        h = torch.arange((-self.scale + 1) / 2, (self.scale - 1) / 2 + 1) / self.scale
        return torch.stack(torch.meshgrid([h, h], indexing="ij")).transpose(1, 2).repeat(1, self.groups, 1).reshape(
            1, -1, 1, 1)

    def emit(self, plan, x, out=None):
        # offset = 0.25 * conv1x1(x) + init_pos  ->  folded into the conv weights/bias (0.25 is exact)
        w = self.offset.weight.detach().float().cpu() * 0.25
        b = self.offset.bias.detach().float().cpu() * 0.25 + self.init_pos.detach().float().cpu().view(-1)
        y = out if out is not None else plan.alloc(x.n, 2 * x.h, 2 * x.w, x.c)
        if (not os.environ.get("YDBL_DS2_OFF") and self.groups == 4 and x.c in (64, 128, 256)
                and vec_aligned(x) and vec_aligned(y)):
            # offset conv + sample in one launch (csrc/dysample2.hip), bit-identical to the pair below; it reads
            # and writes whole 16-byte channel vectors (check_view(need_vec_align) in ydbl_dysample2)
            wd = plan.const(w.reshape(8 * self.groups, x.c).to(plan.dtype))
            bd = plan.const(b)
            d = _lib.DySample2Desc(x.struct(), wd.data_ptr(), bd.data_ptr(), self.groups, y.struct(), _null_view(),
                                   _null_view(), 0.0, 0.0)
            plan.launch("ydbl_dysample2", d, what="DySample.fused", keep=[d, wd, bd])
            plan.note_writer(y, d)
            return y
        off = plan.alloc(x.n, x.h, x.w, 8 * self.groups)
        emit_conv2d(plan, self.offset, x, off, w, b, what="DySample.offset")
        d = _lib.DySampleDesc(x.struct(), off.struct(), self.groups, y.struct(), _null_view(), _null_view(), 0.0, 0.0)
        plan.launch("ydbl_dysample_ex", d, what="DySample.sample", keep=[d])
        plan.note_writer(y, d)  # a FullPAD_Tunnel on y becomes this launch's second output
        return y


class LSKblock(PlanModule):
    """U/nn/modules_attention/LSKA.py:28-52."""

    def __init__(self, dim):
        super().__init__()
        self.conv0 = nn.Conv2d(dim, dim, 5, padding=2, groups=dim)
        self.conv_spatial = nn.Conv2d(dim, dim, 7, stride=1, padding=9, groups=dim, dilation=3)
        self.conv1 = nn.Conv2d(dim, dim // 2, 1)
        self.conv2 = nn.Conv2d(dim, dim // 2, 1)
        self.conv_squeeze = nn.Conv2d(2, 2, 7, padding=3)
        self.conv = nn.Conv2d(dim // 2, dim, 1)

    def emit(self, plan, x, out=None):
        half = self.conv1.out_channels
        a1, a2 = emit_dw_pair(plan, self.conv0, self.conv_spatial, x, what="LSK.dw5+dw7d3")
        y = out if out is not None else plan.alloc(x.n, x.h, x.w, x.c)
        # fused at dim 256 (DBL-n); at 512 (DBL-s) the five launches measured faster in the two-branch layout:
        # DBL-s bs8 per rank +1.6 %, bs64 +0.4 %; DBL-n bs32 fused +1.1 % (profiles/r06/r06_fusion_switch_sweep.txt,
        # r06_sweep2.txt).  YDBL_LSK_FUSE=1 / 0 forces either.
        fuse = os.environ.get("YDBL_LSK_FUSE")
        if (plan.dtype == torch.float16 and x.c in (256, 512) and (fuse == "1" or (fuse is None and x.c == 256))
                and vec_aligned(x) and vec_aligned(y) and y.base is not x.base):
            # conv1 | conv2 + stats, then gate + conv + x * in two launches (csrc/lsk.hip)
            attn = plan.alloc(x.n, x.h, x.w, 2 * half)
            ws = plan.scratch(_lib.lib.ydbl_lsk_gate_workspace(x.n, x.h, x.w))
            c = plan.const
            w12 = c(torch.cat([self.conv1.weight.detach().float().reshape(half, -1),
                               self.conv2.weight.detach().float().reshape(half, -1)], 0).to(plan.dtype).contiguous())
            b12 = c(torch.cat([self.conv1.bias.detach().float(), self.conv2.bias.detach().float()]))
            sw, sb = c(self.conv_squeeze.weight.float()), c(self.conv_squeeze.bias.float())
            wo = c(self.conv.weight.detach().float().reshape(x.c, half).to(plan.dtype).contiguous())
            bo = c(self.conv.bias.detach().float())
            d = _lib.LskDesc(x.struct(), a1.struct(), a2.struct(), attn.struct(), y.struct(), w12.data_ptr(),
                             b12.data_ptr(), sw.data_ptr(), sb.data_ptr(), wo.data_ptr(), bo.data_ptr(), ws.data_ptr())
            keep = [d, ws, w12, b12, sw, sb, wo, bo]
            plan.launch("ydbl_lsk_attn", d, what="LSK.conv12+stats", keep=keep)
            plan.launch("ydbl_lsk_out", d, what="LSK.gate+conv", keep=keep)
            plan.note_writer(y, d)
            return y
        attn = plan.alloc(x.n, x.h, x.w, 2 * half)
        emit_conv2d(plan, self.conv1, a1, attn.cslice(0, half), what="LSK.conv1")
        emit_conv2d(plan, self.conv2, a2, attn.cslice(half, half), what="LSK.conv2")
        gated = plan.alloc(x.n, x.h, x.w, half)
        ws = plan.scratch(_lib.lib.ydbl_lsk_gate_workspace(x.n, x.h, x.w))
        sw = plan.const(self.conv_squeeze.weight.float())
        sb = plan.const(self.conv_squeeze.bias.float())
        plan.launch("ydbl_lsk_gate", attn.struct(), sw.data_ptr(), sb.data_ptr(), gated.struct(), ws.data_ptr(),
                    what="LSK.gate", keep=[sw, sb, ws])
        return emit_conv2d(plan, self.conv, gated, y, res=x, res_mode=_lib.RES_MUL, what="LSK.conv")


# =============================================================================== head
class DFL(nn.Module):
    """U/nn/modules/block.py:65-84 (fixed 0..15 expectation; computed inside ydbl_detect_decode)."""

    def __init__(self, c1=16):
        super().__init__()
        self.conv = nn.Conv2d(c1, 1, 1, bias=False).requires_grad_(False)
        self.conv.weight.data[:] = torch.arange(c1, dtype=torch.float).view(1, c1, 1, 1)
        self.c1 = c1


class Detect(PlanModule):
    """U/nn/modules/head.py:21-198 — per level cat(cv2 box branch, cv3 cls branch); decode in ydbl_detect_decode."""

    dynamic = False
    export = False
    end2end = False
    max_det = 300
    shape = None
    legacy = False

    def __init__(self, nc: int = 80, ch: tuple = (), legacy: bool | None = None):
        super().__init__()
        self.nc = nc
        self.nl = len(ch)
        self.reg_max = 16
        self.no = nc + self.reg_max * 4
        self.stride = torch.zeros(self.nl)
        if legacy is not None:
            self.legacy = legacy
        c2, c3 = max((16, ch[0] // 4, self.reg_max * 4)), max(ch[0], min(self.nc, 100))
        self.cv2 = nn.ModuleList(
            nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * self.reg_max, 1)) for x in ch
        )
        self.cv3 = (
            nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, self.nc, 1)) for x in ch)
            if self.legacy
            else nn.ModuleList(
                nn.Sequential(
                    nn.Sequential(DWConv(x, x, 3), Conv(x, c3, 1)),
                    nn.Sequential(DWConv(c3, c3, 3), Conv(c3, c3, 1)),
                    nn.Conv2d(c3, self.nc, 1),
                )
                for x in ch
            )
        )
        self.dfl = DFL(self.reg_max)

    def bias_init(self):
        """U/nn/modules/head.py:183-194."""
        for a, b, s in zip(self.cv2, self.cv3, self.stride):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[: self.nc] = math.log(5 / self.nc / (640 / s) ** 2)

    def _forward_plan(self, plan, xs):
        """forward(x) in inference mode (head.py:108-118 with export False): the per-level maps x[i] =
        cat(box, cls) and y = _inference(x) (head.py:143-181: DFL, make_anchors, dist2bbox, sigmoid) decoded by
        ydbl_detect_decode into y [B, 4+nc, A] (no candidates: the threshold is above every score).  Returns the
        call's finisher -> (y, [x_i]) as fresh tensors of the plan's dtype."""
        if not float(self.stride.abs().sum()):
            raise RuntimeError("Detect.stride is unset: build the module through DetectionModel (stride probe)")
        levels = self.emit(plan, xs)
        B = levels[0].n
        A = sum(lv.h * lv.w for lv in levels)
        dev = plan.device
        pred = torch.empty((B, 4 + self.nc, A), dtype=torch.float32, device=dev)
        plan.buffers.append(pred)
        dd = decode_desc(levels, self.stride.tolist(), self.nc, self.reg_max, 2.0, False, None, pred,
                         CandidateLists(B, A, dev, plan))
        plan.launch("ydbl_detect_decode", dd, what="Detect.decode", keep=[dd])
        dt = plan.dtype
        return lambda: (pred.to(dt, copy=True), [lv.nchw().contiguous() for lv in levels])

    def emit(self, plan, xs, out=None):
        """Per level: one NHWC buffer [B,h,w,64+nc] (box logits | class logits) = the reference's x[i].  Box branch
        first; a DetectSession on the sparse box path moves the one-launch box branch of a level behind the level's
        class tail once it knows its thresholds (tail.NmsTail.sparse_box)."""
        return self._emit_branches(plan, xs, self.cv2, self.cv3)

    def _emit_branches(self, plan, xs, cv2, cv3):
        """emit() for one set of box / class branches (an end2end head has two)."""
        levels = []
        for i, x in enumerate(xs):
            lv = plan.alloc(x.n, x.h, x.w, self.no)
            if not emit_detect_box(plan, cv2[i], x, lv.cslice(0, 4 * self.reg_max)):
                t = emit_conv3x3_pair(plan, cv2[i][0], cv2[i][1], x)
                emit_conv2d(plan, cv2[i][2], t, lv.cslice(0, 4 * self.reg_max), what="Detect.box")
            if self.legacy:
                u = cv3[i][0].emit(plan, x)
                u = cv3[i][1].emit(plan, u)
            else:  # [DWConv, Conv1x1] x 2: each pair is one fused depthwise -> pointwise launch; the class conv
                # cv3[i][2] (64 -> nc <= 4) rides in the second pair's epilogue, and the pair's own 64-channel
                # output then has no reader (only the class logits leave the launch: y_unused)
                cls_out = lv.cslice(4 * self.reg_max, self.nc)
                u, _ = emit_dw_pw(plan, cv3[i][0][0], cv3[i][0][1], x)
                u, done = emit_dw_pw(plan, cv3[i][1][0], cv3[i][1][1], u, tail_conv=cv3[i][2],
                                     tail_out=cls_out, y_unused=True)
                if done:
                    levels.append(lv)
                    continue
            emit_conv2d(plan, cv3[i][2], u, lv.cslice(4 * self.reg_max, self.nc), what="Detect.cls")
            levels.append(lv)
        return levels


class v10Detect(Detect):  # noqa: N801 (reference name)
    """U/nn/modules/head.py:768-817 (YOLOv10) on Detect.forward_end2end (:120-141) — end2end = True: the class branch is
    Conv(x, x, 3, g=x) -> Conv1x1 (the DWConv pair written as grouped Convs), and one2one_cv2 / one2one_cv3 are deep
    copies of both branch sets.  Inference decodes the ONE2ONE maps, with xyxy boxes (ydbl_detect_decode_e2e), and
    selects with a top-k instead of an NMS (ydbl_detect_topk); max_det = 300 is the head's own, never the
    predictor's.  emit() in a session runs only the one2one branches: the one2many maps have no reader at
    inference.  forward(x) returns the reference's (y [B, min(300, A), 6], {"one2many": [...], "one2one": [...]})."""

    end2end = True
    max_det = 300

    def __init__(self, nc: int = 80, ch: tuple = ()):
        super().__init__(nc, ch)
        self.legacy = False  # the class branch below is the DWConv -> Conv1x1 form whatever the model's flag
        c3 = max(ch[0], min(self.nc, 100))
        self.cv3 = nn.ModuleList(
            nn.Sequential(
                nn.Sequential(Conv(x, x, 3, g=x), Conv(x, c3, 1)),
                nn.Sequential(Conv(c3, c3, 3, g=c3), Conv(c3, c3, 1)),
                nn.Conv2d(c3, self.nc, 1),
            )
            for x in ch
        )
        self.one2one_cv2 = copy.deepcopy(self.cv2)
        self.one2one_cv3 = copy.deepcopy(self.cv3)

    def bias_init(self):
        """U/nn/modules/head.py:183-194: both branch sets."""
        super().bias_init()
        for a, b, s in zip(self.one2one_cv2, self.one2one_cv3, self.stride):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[: self.nc] = math.log(5 / self.nc / (640 / s) ** 2)

    def emit(self, plan, xs, out=None):
        return self._emit_branches(plan, xs, self.one2one_cv2, self.one2one_cv3)

    def _forward_plan(self, plan, xs):
        """forward(x) in inference mode (head.py:120-141 with export False): both branch sets, the one2one maps
        decoded to xyxy (ydbl_detect_decode_e2e) and Detect.postprocess (head.py:200-221) as ydbl_detect_topk with no
        score threshold, no clipping and k = min(max_det, A).  Returns the call's finisher ->
        (y [B, k, 6], {"one2many": [x_i], "one2one": [x_i]}) as fresh tensors of the plan's dtype."""
        if not float(self.stride.abs().sum()):
            raise RuntimeError("Detect.stride is unset: build the module through DetectionModel (stride probe)")
        from ..engine.session import DetectOptions

        many = self._emit_branches(plan, xs, self.cv2, self.cv3)
        one = self.emit(plan, xs)
        B = one[0].n
        A = sum(lv.h * lv.w for lv in one)
        # every (anchor, class) pair a candidate, the head's own cut, boxes unclipped
        opt = DetectOptions(conf=-1.0, max_det=min(self.max_det, A), clip=False)
        tail = E2ETail(plan, B, A, self, opt)
        tail.emit_decode(one)
        tail.emit_topk(0, 0)
        dt = plan.dtype
        return lambda: (tail.det.to(dt, copy=True), {"one2many": [lv.nchw().contiguous() for lv in many],
                                                     "one2one": [lv.nchw().contiguous() for lv in one]})


def emit_deconv2x2(plan: Plan, m: nn.ConvTranspose2d, x: TV, out: TV | None = None, act=_lib.ACT_NONE) -> TV:
    """nn.ConvTranspose2d(c, c, 2, 2, 0) as one ydbl_deconv2x2_nhwc launch; the weight is packed here from torch's
    [cin][cout][2][2] into [2*dy+dx][cout][cin] in the plan dtype (include/ydbl.h)."""
    if (m.kernel_size != (2, 2) or m.stride != (2, 2) or m.padding != (0, 0) or m.output_padding != (0, 0)
            or m.dilation != (1, 1) or m.groups != 1):
        raise NotImplementedError("ConvTranspose2d: only kernel 2, stride 2, pad 0, groups 1 has a HIP kernel")
    if m.in_channels != x.c or m.in_channels % 32 or m.out_channels % 32:
        raise NotImplementedError(f"ConvTranspose2d({m.in_channels}, {m.out_channels}) on {x.c} channels: cin and cout "
                                  "must be multiples of 32")
    y = out if out is not None else plan.alloc(x.n, 2 * x.h, 2 * x.w, m.out_channels)
    wd = plan.const(m.weight.detach().float().cpu().permute(2, 3, 1, 0).contiguous().to(plan.dtype))
    bd = plan.const(m.bias.detach().float().cpu()) if m.bias is not None else None
    d = _lib.DeconvDesc(x.struct(), y.struct(), wd.data_ptr(), bd.data_ptr() if bd is not None else None, act)
    plan.launch("ydbl_deconv2x2_nhwc", d, what="deconv2x2", keep=[wd, bd, d])
    return y


class Proto(PlanModule):
    """U/nn/modules/block.py:87-104 — Conv3x3 -> ConvTranspose2d(c_, c_, 2, 2) -> Conv3x3 -> Conv1x1: the mask
    prototypes at twice the P3 resolution."""

    def __init__(self, c1, c_=256, c2=32):
        super().__init__()
        self.cv1 = Conv(c1, c_, k=3)
        self.upsample = nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True)
        self.cv2 = Conv(c_, c_, k=3)
        self.cv3 = Conv(c_, c2)

    def emit(self, plan, x, out=None):
        t = self.cv1.emit(plan, x)
        t = emit_deconv2x2(plan, self.upsample, t)
        t = self.cv2.emit(plan, t)
        return self.cv3.emit(plan, t, out)


class Segment(Detect):
    """U/nn/modules/head.py:224-271 — Detect plus the mask branch: Proto on the P3 map and, per level, cv4 = Conv3x3 ->
    Conv3x3 -> Conv2d 1x1 giving nm mask coefficients per anchor.  The coefficients go into a buffer of their own per
    level ([B, h, w, nm]), so the level buffers [B, h, w, 64 + nc] the decode and the candidate paths read keep
    their layout.  emit() returns the Detect levels and leaves ``plan.seg = (proto view, [coefficient views])``."""

    def __init__(self, nc: int = 80, nm: int = 32, npr: int = 256, ch: tuple = (), legacy: bool | None = None):
        super().__init__(nc, ch, legacy)
        self.nm = nm
        self.npr = npr
        self.proto = Proto(ch[0], self.npr, self.nm)
        c4 = max(ch[0] // 4, self.nm)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nm, 1)) for x in ch)

    def emit(self, plan, xs, out=None):
        levels = self._emit_branches(plan, xs, self.cv2, self.cv3)
        proto = self.proto.emit(plan, xs[0])
        mcs = []
        for i, x in enumerate(xs):
            t = emit_conv3x3_pair(plan, self.cv4[i][0], self.cv4[i][1], x)
            mcs.append(emit_conv2d(plan, self.cv4[i][2], t, plan.alloc(x.n, x.h, x.w, self.nm), what="Segment.mc"))
        plan.seg = (proto, mcs)
        return levels

    def _forward_plan(self, plan, xs):
        """forward(x) in inference mode (head.py:259-271 with export False): (cat([y, mc], 1) [B, 4+nc+nm, A],
        (feats, mc [B, nm, A], p [B, nm, mh, mw])) as fresh tensors of the plan's dtype."""
        det = super()._forward_plan(plan, xs)
        proto, mcs = plan.seg

        def finish():
            y, feats = det()
            mc = seg_coefficients(mcs)
            return torch.cat([y, mc], 1), (feats, mc, proto.nchw().contiguous())

        return finish


def seg_coefficients(mcs) -> torch.Tensor:
    """The per-level coefficient views [B, h, w, nm] as the reference's mc [B, nm, A] (head.py:264), a fresh tensor."""
    return torch.cat([v.torch().reshape(v.n, v.h * v.w, v.c) for v in mcs], 1).permute(0, 2, 1).contiguous()


def emit_conv_padded(plan: Plan, m: "Conv", x: TV, c_pad: int) -> TV:
    """A Conv whose output channel count is no multiple of 8, carried at c_pad = round_up(c, 8) channels so that the
    next dense conv reads whole 16-byte channel vectors: the extra output channels get zero weight rows and zero bias,
    and SiLU(0) = 0, so they are exact zeros.  m's input may itself be such a padded map (emit_dense's ci < x.c)."""
    conv = m.conv
    assert conv.groups == 1 and conv.out_channels <= c_pad and isinstance(m.act, (nn.SiLU, nn.Identity))
    w, b = m.folded()
    co = conv.out_channels
    if b is None:
        b = torch.zeros(co)
    w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, c_pad - co))
    b = torch.nn.functional.pad(b, (0, c_pad - co))
    k, s, p, d = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
    ho, wo = conv_out_hw(x.h, x.w, k, s, p, d)
    y = plan.alloc(x.n, ho, wo, c_pad)
    emit_dense(plan, x, y, w, b, s, p, d, _act_code(m.act), what=f"Conv{k}x{k}.pad{c_pad}")
    return y


class Pose(Detect):
    """U/nn/modules/head.py:328-401 — Detect plus the keypoint branch: per level cv4 = Conv3x3 -> Conv3x3 -> Conv2d 1x1
    giving nk = K * ndim raw keypoint values per anchor.  They go into a buffer of their own per level
    ([B, h, w, nk]), so the level buffers [B, h, w, 64 + nc] keep their layout and the boxes equal the detection
    model's.  emit() returns the Detect levels and leaves ``plan.pose = [keypoint views]``; the kept rows' keypoints
    are decoded behind the NMS by ydbl_pose_keypoints (tail.NmsTail).  c4 = max(ch[0] // 4, nk) need not be a multiple
    of 8 (51 at scales n and s): the two 3x3 intermediates are then carried zero-padded (emit_conv_padded)."""

    def __init__(self, nc: int = 80, kpt_shape: tuple = (17, 3), ch: tuple = (), legacy: bool | None = None):
        super().__init__(nc, ch, legacy)
        self.kpt_shape = kpt_shape
        self.nk = kpt_shape[0] * kpt_shape[1]
        c4 = max(ch[0] // 4, self.nk)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nk, 1)) for x in ch)

    def emit(self, plan, xs, out=None):
        levels = self._emit_branches(plan, xs, self.cv2, self.cv3)
        kpts = []
        for i, x in enumerate(xs):
            c4 = self.cv4[i][0].conv.out_channels
            if c4 % 8:
                t = emit_conv_padded(plan, self.cv4[i][0], x, round_up(c4, 8))
                t = emit_conv_padded(plan, self.cv4[i][1], t, round_up(c4, 8))
            else:
                t = emit_conv3x3_pair(plan, self.cv4[i][0], self.cv4[i][1], x)
            kpts.append(emit_conv2d(plan, self.cv4[i][2], t, plan.alloc(x.n, x.h, x.w, self.nk), what="Pose.kpt"))
        plan.pose = kpts
        return levels

    def _forward_plan(self, plan, xs):
        """forward(x) in inference mode (head.py:364-372 with export False): (cat([y, pred_kpt], 1) [B, 4+nc+nk, A],
        (feats, kpt [B, nk, A])) as fresh tensors of the plan's dtype; kpts_decode in torch, as the reference's."""
        det = super()._forward_plan(plan, xs)
        kpts, strides = plan.pose, self.stride.tolist()

        def finish():
            y, feats = det()
            kpt = pose_raw(kpts).to(y.dtype)
            return torch.cat([y, kpts_decode(kpt, kpts, strides, self.kpt_shape[1])], 1), (feats, kpt)

        return finish


def pose_raw(kpts) -> torch.Tensor:
    """The per-level raw keypoint views [B, h, w, nk] as the reference's kpt [B, nk, A] (head.py:367), a fresh tensor."""
    return torch.cat([v.torch().reshape(v.n, v.h * v.w, v.c) for v in kpts], 1).permute(0, 2, 1).contiguous()


def pose_grid(kpts, strides, device):
    """(gx [A], gy [A], stride [A]) fp32 of the anchors of the levels `kpts` (views or (h, w) pairs), level after
    level, row-major: make_anchors' points minus 0.5 (U/utils/tal.py:317-330)."""
    gx, gy, st = [], [], []
    for v, s in zip(kpts, strides):
        h, w = (v.h, v.w) if hasattr(v, "h") else v
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device),
                                torch.arange(w, dtype=torch.float32, device=device), indexing="ij")
        gx.append(xx.reshape(-1))
        gy.append(yy.reshape(-1))
        st.append(torch.full((h * w,), float(s), dtype=torch.float32, device=device))
    return torch.cat(gx), torch.cat(gy), torch.cat(st)


def kpts_decode(kpt: torch.Tensor, kpts, strides, ndim: int) -> torch.Tensor:
    """Pose.kpts_decode (head.py:396-401) of kpt [B, nk, A] in kpt's dtype, in torch: the parity surface of
    ``model(x)``, not the hot path (ydbl_pose_keypoints decodes the kept rows)."""
    gx, gy, st = (t.to(kpt.dtype) for t in pose_grid(kpts, strides, kpt.device))
    y = kpt.clone()
    if ndim == 3:
        y[:, 2::3] = y[:, 2::3].sigmoid()
    y[:, 0::ndim] = (y[:, 0::ndim] * 2.0 + gx) * st
    y[:, 1::ndim] = (y[:, 1::ndim] * 2.0 + gy) * st
    return y


def emit_module(m: nn.Module, plan: Plan, x, out=None):
    """Emit any parsed layer: built-in modules (HIP launches), nn.Sequential repeats, and registered plugin
    classes that only have a torch forward (emit_torch)."""
    if isinstance(m, nn.Sequential):
        return emit_seq(plan, m, x, out)
    if hasattr(m, "emit"):
        return m.emit(plan, x, out)
    if type(m).forward is not nn.Module.forward:
        return emit_torch(m, plan, x, out)
    raise NotImplementedError(f"{type(m).__name__} has neither emit() nor forward()")
