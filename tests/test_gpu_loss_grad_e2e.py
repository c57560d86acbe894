"""The differentiable criterion end to end on the GPU: ``v8DetectionLoss`` of a DBL-n model object (nc 3; only its
strides and gains matter) over the level maps of a tiny torch head, so that torch autograd runs through
ydbl_detect_loss_grad into the head's weights.

The head: fixed random features X_l [2, 16, h_l, w_l] for a 64 x 96 input, one parameter W_l [67, 16] ~ 0.5 N(0, 1)
per level, a bias of 0 on the box channels and -2 on the class channels; level maps einsum('bchw,oc->bohw') + bias --
contiguous NCHW, what a torch Detect in train mode produces, so the criterion's channels-last copy path runs and the
gradient reaches the einsum through a strided view.  Labels: loss_util.synthetic_case.

Reference: tests/loss_grad_util.py in fp64 through the same einsum, fed the device's assignment (a second, plain
forward over the same maps: the kernel is bit-reproducible).  Under autocast the restatement takes the fp16 values the
criterion read (straight-through to the fp64 einsum of the fp16-rounded operands).  Bound: that of
tests/test_gpu_loss_grad.py -- 32 x the restatement's fp32-to-fp64 yardstick relative to the largest |gradient|, box
and class rows apart, plus 2^-11 |ref| + 2^-24 per fp16 element -- on the level-map gradients and, in fp32, taken on
W.grad; under autocast W.grad gets that bound carried through the einsum (test_..._autocast says why).
"""

import pytest
import torch

from loss_grad_util import given_assignment_loss
from loss_util import GAINS, rel_dist, synthetic_case
from test_gpu_loss_grad import FACTOR, yardstick

pytestmark = pytest.mark.gpu

B, H, W, NC, CIN = 2, 64, 96, 3, 16
STRIDES = [8, 16, 32]
SHAPES = [(H // s, W // s) for s in STRIDES]


@pytest.fixture(scope="module")
def crit():
    from ydbl import YOLO

    return YOLO("yolov13n_DBL.yaml", nc=NC).model.init_criterion()


def make_batch(seed):
    """The labels of synthetic_case(seed) for two images as a reference batch dict (normalised xywh)."""
    _, _, _, gt = synthetic_case(seed, h=H, w=W, nc=NC, counts=(6, 3))
    rows = [(b, gt[b, m]) for b in range(B) for m in range(gt.shape[1]) if float(gt[b, m, 1:].sum()) > 0]
    bidx = torch.tensor([float(b) for b, _ in rows])
    cls = torch.stack([r[0] for _, r in rows]).view(-1, 1)
    xyxy = torch.stack([r[1:] for _, r in rows])
    xywh = torch.cat(((xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]), 1) / torch.tensor([W, H, W, H])
    return {"batch_idx": bidx, "cls": cls, "bboxes": xywh}


class Head:
    def __init__(self, seed, device):
        gen = torch.Generator().manual_seed(1000 + seed)
        self.x = [torch.randn(B, CIN, h, w, generator=gen).to(device) for h, w in SHAPES]
        self.w = [(0.5 * torch.randn(64 + NC, CIN, generator=gen)).to(device).requires_grad_(True) for _ in SHAPES]
        self.bias = torch.cat((torch.zeros(64), torch.full((NC,), -2.0))).to(device)

    def feats(self, x=None, w=None, bias=None, channels_last=False):
        """Contiguous NCHW level maps (the criterion copies them to channels-last), or channels-last ones (read in
        place)."""
        x, w, bias = x or self.x, w or self.w, self.bias if bias is None else bias
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        out = []
        for xl, wl in zip(x, w):
            f = torch.einsum("bchw,oc->bohw", xl, wl)
            out.append((f + bias.to(f.dtype)[None, :, None, None]).contiguous(memory_format=fmt))
        return out


def device_assignment(crit, feats, batch):
    """A plain forward over the same level maps with the assignment kept, read back to the CPU."""
    from ydbl.utils.loss import LossBuffers, level_views

    gt = crit.preprocess(batch, B, (H, W))
    boxes, clss, keep = level_views([f.detach() for f in feats])
    bufs = LossBuffers(boxes, clss, crit.stride, crit.nc, crit.gains, crit.max_labels, crit.tal_topk, keep[0].device,
                       debug=True)
    bufs.gt.copy_(gt)
    bufs.launch()
    torch.cuda.synchronize()
    return gt, (bufs.fg.cpu().bool(), bufs.target_gt_idx.cpu().long(), bufs.target_score.cpu(),
                bufs.target_scores_sum.cpu().reshape(()))


def reference_grads(head, dev_feats, gt, assignment, half):
    """(d(total)/dW_l, d(total)/d(level map l)) by fp64 autograd through the einsum.  half: the operands rounded to
    fp16 as autocast feeds them, the level values the fp16 ones the criterion read (straight-through)."""
    rnd = (lambda t: t.detach().cpu().half().double()) if half else (lambda t: t.detach().cpu().double())
    w = [rnd(t).requires_grad_(True) for t in head.w]
    feats = head.feats([rnd(t) for t in head.x], w, head.bias.cpu().double())
    if half:
        feats = [f + (d.detach().cpu().double() - f).detach() for f, d in zip(feats, dev_feats)]
    flat = torch.cat([f.flatten(2).permute(0, 2, 1) for f in feats], 1)
    total, _ = given_assignment_loss(flat[..., :64], flat[..., 64:], SHAPES, STRIDES, gt, *assignment, GAINS,
                                     torch.float64)
    grads = torch.autograd.grad(total, [*w, *feats])
    return grads[:len(w)], grads[len(w):]


def element_bound(ref, yard, f16, dim):
    """The bound of tests/test_gpu_loss_grad.py per element of a gradient whose axis ``dim`` holds the 64 box and the
    nc class channels, the two groups apart: 32 x yardstick x max|ref| (+ 2^-11 |ref| + 2^-24 for an fp16 value)."""
    groups = (("box", ref.narrow(dim, 0, 64)), ("cls", ref.narrow(dim, 64, ref.shape[dim] - 64)))
    return torch.cat([FACTOR * yard[k] * r.abs().max() + ((2.0**-11) * r.abs() + 2.0**-24 if f16 else torch.zeros_like(r))
                      for k, r in groups], dim)


def check(what, got, ref, tol):
    err = (got.detach().cpu().double() - ref).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{what}: rel_dist {rel_dist(got.detach().cpu(), ref):.3g} worst |err| / bound {worst:.3g} max|ref| "
          f"{float(ref.abs().max()):.3g}")
    assert bool((err <= tol).all()), (what, worst)
    return worst


def test_backward_fills_the_head_weights_fp32(crit):
    """W.grad against the fp64 restatement under the kernel test's bound, taken on W.grad (box and class rows apart);
    the level-map gradients the einsum received under the same bound."""
    dev = torch.device("cuda", 0)
    head, batch = Head(0, dev), make_batch(0)
    feats = head.feats()
    for f in feats:
        f.retain_grad()
    total, items = crit(feats, batch)
    assert feats[0].dtype == torch.float32 and feats[0].is_contiguous()
    assert total.grad_fn is not None and total.dtype == torch.float32
    total.backward()
    torch.cuda.synchronize()
    gt, assignment = device_assignment(crit, feats, batch)
    assert int(assignment[0].sum()) > 0
    wref, fref = reference_grads(head, feats, gt, assignment, False)
    y = yardstick()
    for l, (w, f) in enumerate(zip(head.w, feats)):
        assert w.grad is not None and w.grad.shape == w.shape and bool(torch.isfinite(w.grad).all())
        assert f.grad.shape == f.shape and f.grad.dtype == f.dtype
        check(f"fp32 level {l} gradient", f.grad, fref[l], element_bound(fref[l], y, False, 1))
        check(f"fp32 W{l}.grad", w.grad, wref[l], element_bound(wref[l], y, False, 0))


def test_backward_fills_the_head_weights_autocast(crit):
    """The same under torch.autocast(dtype=torch.float16) with a scale of 1024 on the loss.  The level maps are fp16
    and are read as they are; the gradient views are fp16, rounded once after the scale.

    The level-map gradients meet the kernel test's fp16 bound element by element.  W.grad cannot meet that bound
    taken literally on W.grad: the einsum's backward sums up to 192 products g_i x_i whose g_i each carry their own
    2^-11 rounding, which do not cancel where the sum does.  Fed the EXACT fp64 gradients rounded once to fp16 (an
    ideal kernel) and an exact sum, the literal bound is missed by up to 1.2 x / 4.9 x / 2.8 x on levels 0 / 1 / 2 of
    this head (CPU; with an fp16 matmul output 1.4 x / 4.9 x / 3.3 x); this kernel behind torch's fp16 einsum backward
    on the MI355X: 4.1 x / 14.4 x / 3.9 x.  W.grad is therefore held to the same element bound carried through the
    einsum, which is linear in g:
    sum_i |x_i| bound(g_i), plus one fp16 rounding of the matmul's output, 2^-11 |ref| + 2^-24 (in the scaled
    domain).  The ratio to the literal bound is printed."""
    dev = torch.device("cuda", 0)
    head, batch = Head(0, dev), make_batch(0)
    scale = 1024.0
    with torch.autocast("cuda", dtype=torch.float16):
        feats = head.feats()
        for f in feats:
            f.retain_grad()
        total, items = crit(feats, batch)
    assert feats[0].dtype == torch.float16 and feats[0].is_contiguous()
    assert total.grad_fn is not None and total.dtype == torch.float32
    (total * scale).backward()
    torch.cuda.synchronize()
    gt, assignment = device_assignment(crit, feats, batch)
    assert int(assignment[0].sum()) > 0
    wref, fref = reference_grads(head, feats, gt, assignment, True)
    y = yardstick()
    for l, (w, f) in enumerate(zip(head.w, feats)):
        assert w.grad is not None and w.grad.dtype == torch.float32 and bool(torch.isfinite(w.grad).all())
        assert f.grad.shape == f.shape and f.grad.dtype == torch.float16
        g_ref, w_ref = scale * fref[l], scale * wref[l]
        g_tol = element_bound(g_ref, y, True, 1)
        check(f"autocast level {l} gradient x 1024", f.grad, g_ref, g_tol)
        x16 = head.x[l].detach().cpu().half().double().abs()
        w_tol = torch.einsum("bohw,bchw->oc", g_tol, x16) + (2.0**-11) * w_ref.abs() + 2.0**-24
        check(f"autocast W{l}.grad x 1024", w.grad, w_ref, w_tol)
        literal = element_bound(w_ref, y, True, 0)
        print(f"autocast W{l}.grad x 1024: worst |err| / the bound taken literally on W.grad "
              f"{float(((w.grad.cpu().double() - w_ref).abs() / literal).max()):.3g}")


def test_once_differentiable_and_detached_items(crit):
    dev = torch.device("cuda", 0)
    head, batch = Head(1, dev), make_batch(1)
    total, items = crit(head.feats(), batch)
    assert not items.requires_grad and items.grad_fn is None
    total.backward()
    with pytest.raises(RuntimeError):
        total.backward()  # the saved tensors are gone
    total, _ = crit(head.feats(), batch)
    g = torch.autograd.grad(total, head.w, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(sum(x.sum() for x in g), head.w)  # double backward


def test_forward_is_unchanged_without_grad(crit):
    dev = torch.device("cuda", 0)
    head, batch = Head(2, dev), make_batch(2)
    feats = head.feats()
    total, items = crit(feats, batch)
    tss, per = crit.target_scores_sum.clone(), crit.per_image.clone()
    assert total.grad_fn is not None
    t0, i0 = crit([f.detach() for f in feats], batch)
    assert t0.grad_fn is None and not t0.requires_grad and not i0.requires_grad
    assert torch.equal(t0, total.detach()) and torch.equal(i0, items)
    assert torch.equal(crit.target_scores_sum, tss) and torch.equal(crit.per_image, per)
    with torch.no_grad():
        t1, i1 = crit(feats, batch)
    assert t1.grad_fn is None and not t1.requires_grad
    assert torch.equal(t1, total.detach()) and torch.equal(i1, items)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sgd_lowers_the_loss(crit, seed):
    """60 steps of plain SGD on the head's weights, W <- W - (0.02 / B) W.grad of the total: the largest
    loss_items.sum() of the last 10 steps is below 0.85 x the first step's.  The same loop on the CPU with the
    restated gradients (this file's head and labels, the restated assigner) gave 100.9 -> 37.3 (largest of the last
    10: 37.6), 77.8 -> 24.0 (26.2) and 132.7 -> 30.8 (38.0) for seeds 0, 1, 2: a wide margin for a correct gradient,
    a failure for a sign or scale error."""
    dev = torch.device("cuda", 0)
    head, batch = Head(seed, dev), make_batch(seed)
    sums = []
    for _ in range(60):
        total, items = crit(head.feats(channels_last=seed == 1), batch)  # seed 1: maps the criterion reads in place
        total.backward()
        with torch.no_grad():
            for w in head.w:
                w -= (0.02 / B) * w.grad
                w.grad = None
        sums.append(items.sum())
    sums = torch.stack(sums).cpu()
    print(f"sgd seed {seed}: loss_items.sum() {float(sums[0]):.1f} -> {float(sums[-1]):.1f}, largest of the last 10 "
          f"{float(sums[-10:].max()):.1f}")
    assert bool(torch.isfinite(sums).all())
    assert float(sums[-10:].max()) < 0.85 * float(sums[0])
