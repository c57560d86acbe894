"""ydbl_detect_loss_grad on the device against torch autograd over the given-assignment restatement
(tests/loss_grad_util.py), directly over NHWC buffers as tests/test_gpu_loss.py runs the forward -- no model.

Each case runs the forward with the assignment kept, then the gradient kernel, reads the DEVICE's assignment back and
feeds it to the restatement, so the code under test is the backward alone (assignment parity: test_gpu_loss.py).
Shapes are the smallest that take every path: three levels, A = 126 and 315 (one and two workgroups of 256 rows, the
second ragged), a level of one cell, an empty image, no labels at all, nc = 1 / 3 (the element-wise class tail) and 80
(whole 8-class groups), pitch 67 (pixels 2-byte aligned: 16-byte accesses at element alignment) and 72 / 144 (every
8-channel group 16-byte aligned), fp32 and fp16 on either side.

Tolerance, separately for the box and the class gradients: the yardstick is the restatement's own fp32-to-fp64
distance on the CPU (rel_dist: relative to the largest |gradient|), the largest over this file's cases; the kernel
gets 32 x that against the fp64 gradient, the factor and yardstick of test_gpu_loss.py.  An fp16 output adds, per
element, 2^-11 |ref| + 2^-24 for its one rounding.  Distances seen on the MI355X:
profiles/r19/r19_loss_grad_parity.txt.
"""

import ctypes as C
import functools

import pytest
import torch

from loss_grad_util import given_assignment_grads
from loss_util import GAINS, flatten_levels, rel_dist, synthetic_case
from test_gpu_loss import run_device, special_case

pytestmark = pytest.mark.gpu

FACTOR = 32.0
SENTINEL = -77.0


def build_cases():
    cases = {}
    for seed in range(4):
        cases[f"base-{seed}"] = (synthetic_case(seed), torch.float32)
        cases[f"half-{seed}"] = (synthetic_case(seed), torch.float16)
    cases["nc80"] = (synthetic_case(1, nc=80), torch.float32)
    cases["nc80-half"] = (synthetic_case(1, nc=80), torch.float16)
    cases["nc1"] = (synthetic_case(2, nc=1), torch.float32)
    cases["96x160"] = (synthetic_case(5, h=96, w=160), torch.float32)
    cases["32x32"] = (synthetic_case(4, h=32, w=32, counts=(2, 0)), torch.float32)
    cases["special"] = (special_case(), torch.float32)
    levels, shapes, strides, gt = synthetic_case(0)
    cases["empty"] = ((levels, shapes, strides, torch.zeros_like(gt)), torch.float32)
    return cases


class Case:
    """The inputs, the device's assignment for them and the restatement's gradients for that assignment."""

    def __init__(self, name, inputs, dtype):
        levels, self.shapes, self.strides, self.gt = inputs
        self.name, self.dtype = name, dtype
        self.levels = [lv.to(dtype) for lv in levels]  # what the device reads; the restatement gets the same values
        self.box, self.cls = flatten_levels([lv.float() for lv in self.levels])
        self.nc = self.cls.shape[-1]
        bufs, _ = run_device(self)
        self.assignment = (bufs.fg.cpu().bool(), bufs.target_gt_idx.cpu().long(), bufs.target_score.cpu(),
                           bufs.target_scores_sum.cpu().reshape(()))
        args = (self.box, self.cls, self.shapes, self.strides, self.gt, *self.assignment, GAINS)
        self.gb64, self.gc64, _ = given_assignment_grads(*args, dtype=torch.float64)
        gb32, gc32, _ = given_assignment_grads(*args, dtype=torch.float32)
        self.yard = {"box": rel_dist(gb32, self.gb64), "cls": rel_dist(gc32, self.gc64)}


@functools.lru_cache(maxsize=None)
def all_cases():
    """The references, computed once per session (tests/test_gpu_loss_grad_e2e.py takes its yardstick from here)."""
    return {k: Case(k, inp, dt) for k, (inp, dt) in build_cases().items()}


def yardstick():
    cs = all_cases().values()
    return {k: max(c.yard[k] for c in cs) for k in ("box", "cls")}


def run_grad(case, in_pad=0, g_pad=0, g_dtype=None, scale=None, batch_scale=None):
    """Forward with the assignment kept, then one ydbl_detect_loss_grad launch over [B, h, w, 64+nc(+pad)] buffers.
    Returns (gbox [B, A, 64], gcls [B, A, nc]) on the CPU in the gradient dtype; asserts the pad lanes untouched."""
    from ydbl import _lib

    g_dtype = g_dtype or case.dtype
    bufs, keep = run_device(case, pad=in_pad)  # NaN in the input pad lanes
    dev = keep[0].device
    d = _lib.LossGradDesc()
    d.nl, d.nc, d.reg_max, d.max_labels = len(keep), case.nc, 16, case.gt.shape[1]
    d.gain_box, d.gain_cls, d.gain_dfl = GAINS
    d.gt, d.fg, d.target_gt_idx = bufs.gt.data_ptr(), bufs.fg.data_ptr(), bufs.target_gt_idx.data_ptr()
    d.target_score, d.target_scores_sum = bufs.target_score.data_ptr(), bufs.target_scores_sum.data_ptr()
    B = keep[0].shape[0]
    d.batch_scale = float(B if batch_scale is None else batch_scale)
    sc = None
    if scale is not None:
        sc = torch.tensor([float(scale)], dtype=torch.float32, device=dev)
        d.grad_scale = sc.data_ptr()
    grads = []
    for i, buf in enumerate(keep):
        _, h, w, pitch = buf.shape
        c = 64 + case.nc
        g = torch.full((B, h, w, c + g_pad), SENTINEL, dtype=g_dtype, device=dev)
        grads.append(g)
        dt, es = _lib.dtype_code(case.dtype), buf.element_size()
        gdt, ges = _lib.dtype_code(g_dtype), g.element_size()
        d.box[i] = _lib.View(buf.data_ptr(), B, h, w, 64, pitch, dt)
        d.cls[i] = _lib.View(buf.data_ptr() + 64 * es, B, h, w, case.nc, pitch, dt)
        d.gbox[i] = _lib.View(g.data_ptr(), B, h, w, 64, c + g_pad, gdt)
        d.gcls[i] = _lib.View(g.data_ptr() + 64 * ges, B, h, w, case.nc, c + g_pad, gdt)
        d.stride[i] = float(case.strides[i])
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib.ydbl_detect_loss_grad(C.byref(d), s), "ydbl_detect_loss_grad")
    torch.cuda.synchronize(dev)
    flat = torch.cat([g.cpu().reshape(B, -1, g.shape[-1]) for g in grads], 1)
    c = 64 + case.nc
    assert bool((flat[..., c:] == SENTINEL).all()), "a pad lane of a gradient buffer was written"
    return flat[..., :64].contiguous(), flat[..., 64:c].contiguous()


def check_close(name, what, got, ref, yard, f16):
    """|got - ref| <= 32 x yardstick x max|ref| (+ 2^-11 |ref| + 2^-24 per element for an fp16 output)."""
    ref = ref.double()
    tol = FACTOR * yard * ref.abs().max() + ((2.0**-11) * ref.abs() + 2.0**-24 if f16 else 0.0)
    err = (got.double() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max()) if ref.numel() else 0.0
    print(f"{name}: {what} rel_dist {rel_dist(got, ref):.3g} (32 x yardstick {FACTOR * yard:.3g}"
          f"{', + the fp16 rounding' if f16 else ''}) worst |err| / bound {worst:.3g} max|ref| {float(ref.abs().max()):.3g}")
    assert bool((err <= tol).all()), (name, what, worst)


NAMES = sorted(build_cases())


@pytest.mark.parametrize("name", NAMES)
def test_grad_matches_autograd(name):
    c, y = all_cases()[name], yardstick()
    gb, gc = run_grad(c)
    f16 = c.dtype == torch.float16
    fg = c.assignment[0]
    print(f"{name}: fg {int(fg.sum())} yardstick box {y['box']:.3g} cls {y['cls']:.3g} (own {c.yard['box']:.3g} "
          f"{c.yard['cls']:.3g})")
    check_close(name, "box", gb, c.gb64, y["box"], f16)
    check_close(name, "cls", gc, c.gc64, y["cls"], f16)
    # rows of anchors that are not foreground: bit-exact zeros (+0)
    rows = gb[~fg]
    assert bool((rows.view(torch.int16 if f16 else torch.int32) == 0).all())
    if name != "empty":
        assert int(fg.sum()) > 0 and float(gb[fg].abs().max()) > 0


def test_no_labels_at_all():
    """Every box gradient is exactly 0 and the class gradients are K * gain_cls * sigmoid(x) (S = max(0, 1) = 1)."""
    c, y = all_cases()["empty"], yardstick()
    assert not bool(c.assignment[0].any()) and float(c.assignment[3]) == 1.0
    gb, gc = run_grad(c)
    assert bool((gb.view(torch.int32) == 0).all())
    want = c.cls.shape[0] * GAINS[1] * c.cls.double().sigmoid()
    check_close("empty", "cls vs K gain sigmoid", gc, want, y["cls"], False)


def test_special_labels():
    """A duplicated label and a 2 x 2 px box without an anchor: the gradient follows the device's assignment."""
    c = all_cases()["special"]
    fg, tgi = c.assignment[0], c.assignment[1]
    assert int((fg[1] & (tgi[1] == 0)).sum()) > 0
    assert int((fg[1] & (tgi[1] == 1)).sum()) == 0 and int((fg[1] & (tgi[1] == 2)).sum()) == 0
    gb, _ = run_grad(c)
    assert float(gb[1][fg[1]].abs().max()) > 0 and float(gb[2].abs().max()) == 0.0  # image 2 has no labels


@pytest.mark.parametrize("name", ["base-3", "half-3", "nc80", "nc80-half"])
def test_bit_identical_and_pitch_independent(name):
    """Two runs give the same bits, and so does every pitch: the input at c and c + 5 (NaN in the pad), the gradient
    at a pitch of its own.  c + 5 = 72 for nc = 3: every 8-channel group 16-byte aligned, against pitch 67."""
    c = all_cases()[name]
    a = run_grad(c)
    for kw in ({}, {"in_pad": 5}, {"g_pad": 5}, {"in_pad": 5, "g_pad": 13}, {"in_pad": 3, "g_pad": 8}):
        b = run_grad(c, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), kw
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())


@pytest.mark.parametrize("name,g_dtype", [("base-1", torch.float16), ("half-1", torch.float32),
                                          ("nc80", torch.float16), ("nc80-half", torch.float32)])
def test_gradient_dtype_differs_from_input(name, g_dtype):
    c, y = all_cases()[name], yardstick()
    f16 = g_dtype == torch.float16
    for kw in ({}, {"in_pad": 5, "g_pad": 5}):
        gb, gc = run_grad(c, g_dtype=g_dtype, **kw)
        assert gb.dtype == g_dtype
        check_close(name, f"box -> {g_dtype}", gb, c.gb64, y["box"], f16)
        check_close(name, f"cls -> {g_dtype}", gc, c.gc64, y["cls"], f16)
    if f16:  # the fp32 value, rounded once: the fp32-output run rounded on the host gives the same bits
        fb, fc = run_grad(c, g_dtype=torch.float32)
        assert torch.equal(fb.half(), gb) and torch.equal(fc.half(), gc)


def test_grad_scale():
    """grad_scale multiplies in fp32, before the one rounding.  fp16, 1024: the result is the fp32-output run's
    value rounded to fp16, and differs from 1024 x the rounded unscaled gradient (whose small values were lost).
    fp32, 3: three times the gradient.  batch_scale enters K the same way."""
    y = yardstick()
    c = all_cases()["half-0"]
    gb, gc = run_grad(c, scale=1024.0)
    check_close("half-0", "box x 1024", gb, 1024.0 * c.gb64, y["box"], True)
    check_close("half-0", "cls x 1024", gc, 1024.0 * c.gc64, y["cls"], True)
    fb, fc = run_grad(c, scale=1024.0, g_dtype=torch.float32)
    assert torch.equal(fb.half(), gb) and torch.equal(fc.half(), gc)
    ub, uc = run_grad(c)
    lost = ((ub.float() * 1024.0) != gb.float()).sum() + ((uc.float() * 1024.0) != gc.float()).sum()
    print(f"half-0: {int(lost)} of {ub.numel() + uc.numel()} fp16 gradients differ from 1024 x the unscaled rounded one")
    assert int(lost) > 0
    c = all_cases()["base-0"]
    gb, gc = run_grad(c, scale=3.0)
    check_close("base-0", "box x 3", gb, 3.0 * c.gb64, y["box"], False)
    check_close("base-0", "cls x 3", gc, 3.0 * c.gc64, y["cls"], False)
    B = c.cls.shape[0]
    hb, hc = run_grad(c, batch_scale=1.0)  # K = 1: the gradient of loss.sum() itself
    check_close("base-0", "box, batch_scale 1", hb, c.gb64 / B, y["box"], False)
    check_close("base-0", "cls, batch_scale 1", hc, c.gc64 / B, y["cls"], False)
