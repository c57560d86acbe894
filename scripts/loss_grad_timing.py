"""What the differentiable criterion costs: DBL-n's level maps at 640 x 640 (80^2 / 40^2 / 20^2 cells, 64 + 3 channels),
batch 32, nc 3, fp16, 8 random labels per image, contiguous NCHW maps (what a torch Detect in train mode hands over: the
criterion's channels-last copy is part of the cost) and channels-last maps (read in place).

Legs, alternated inside one process, median over --reps of the host wall time around work that ends in a device
synchronise:
  forward        criterion(feats, batch) with maps that do not require grad (five launches);
  forward+back   the same with maps that require grad, then total.backward() (six launches);
  eager          forward + backward of tests/loss_grad_util.given_assignment_loss in eager PyTorch on the same GPU,
                 fp32 over the same maps, FED THE SAME ASSIGNMENT: it leaves out the TaskAlignedAssigner (topk /
                 scatter / where and their launches), so it understates what a trainer pays for the torch criterion.
And the gradient launch alone: device events around --inner back-to-back ydbl_detect_loss_grad launches, replayed
from one captured graph and enqueued from Python, next to its byte floor (include/ydbl.h: the box logits of a
non-foreground anchor are not read).

    python scripts/loss_grad_timing.py [--reps 30] [--inner 50] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "yolo-dbl_amd"))
sys.path.insert(0, str(ROOT / "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402

from loss_grad_util import given_assignment_loss  # noqa: E402
from loss_util import random_labels  # noqa: E402
from ydbl import YOLO, _lib  # noqa: E402
from ydbl.utils.loss import LossBuffers, LossGradBuffers, level_views  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
B, S, NC, LABELS = 32, 640, 3, 8
STRIDES = [8, 16, 32]
SHAPES = [(S // s, S // s) for s in STRIDES]
A = sum(h * w for h, w in SHAPES)
HBM = 6.3e12  # B/s, the guide's streaming ceiling
dev = torch.device("cuda", 0)
gen = torch.Generator().manual_seed(0)
crit = YOLO("yolov13n_DBL.yaml", nc=NC).model.init_criterion()
nchw = [torch.cat((2.0 * torch.randn(B, 64, h, w, generator=gen), 1.5 * torch.randn(B, NC, h, w, generator=gen) - 2.0),
                  1).to(dev).half() for h, w in SHAPES]
nhwc = [f.contiguous(memory_format=torch.channels_last) for f in nchw]
gt = random_labels(gen, (LABELS,) * B, S, S, LABELS, NC)
rows = [(b, gt[b, m]) for b in range(B) for m in range(LABELS)]
xyxy = torch.stack([r[1:] for _, r in rows])
batch = {"batch_idx": torch.tensor([float(b) for b, _ in rows]), "cls": torch.stack([r[0] for _, r in rows]),
         "bboxes": torch.cat(((xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]), 1) / S}

# the assignment of these maps, once, for the eager leg and the bare launch
boxes, clss, keep = level_views(nhwc)
fwd = LossBuffers(boxes, clss, crit.stride, NC, crit.gains, crit.max_labels, crit.tal_topk, dev, debug=True)
fwd.gt.copy_(crit.preprocess(batch, B, (S, S)))
fwd.launch()
torch.cuda.synchronize()
n_fg = int(fwd.fg.sum())
flat32 = torch.cat([f.float().flatten(2).permute(0, 2, 1) for f in nchw], 1)


def leg_forward(maps):
    total, _ = crit([f.detach() for f in maps], batch)
    return total


def leg_forward_backward(maps):
    leaves = [f.detach().requires_grad_(True) for f in maps]
    total, _ = crit(leaves, batch)
    total.backward()
    return leaves[0].grad


def leg_eager(_):
    box = flat32[..., :64].detach().requires_grad_(True)
    cls = flat32[..., 64:].detach().requires_grad_(True)
    total, _ = given_assignment_loss(box, cls, SHAPES, STRIDES, fwd.gt, fwd.fg, fwd.target_gt_idx, fwd.target_score,
                                     fwd.target_scores_sum, crit.gains, torch.float32)
    total.backward()
    return box.grad


legs = [("forward, NCHW maps", leg_forward, nchw), ("forward+back, NCHW maps", leg_forward_backward, nchw),
        ("forward, channels-last", leg_forward, nhwc), ("forward+back, channels-last", leg_forward_backward, nhwc),
        ("eager restatement fwd+back", leg_eager, None)]


def timed(fn, arg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(arg)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for _ in range(3):  # warm every leg
    for _, fn, arg in legs:
        timed(fn, arg)
times = {name: [] for name, _, _ in legs}
for r in range(args.reps):  # the cycle starts one leg later each repetition
    k = r % len(legs)
    for name, fn, arg in legs[k:] + legs[:k]:
        times[name].append(timed(fn, arg))

# the gradient launch alone, in-stream, at a dense gradient pitch (64 + nc) and at one rounded up to 8 elements
one = torch.ones(1, dtype=torch.float32, device=dev)


def stream_us(run):
    """Median / min / max device time per launch of ``run`` (which enqueues --inner launches), by events."""
    out = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / args.inner * 1e3)
    return statistics.median(out), min(out), max(out)


def measure(pitch_align):
    gb = LossGradBuffers(keep, crit.stride, NC, crit.gains, fwd.gt, fwd.fg, fwd.target_gt_idx, fwd.target_score,
                         fwd.target_scores_sum, float(B), one, pitch_align=pitch_align)

    def direct():
        for _ in range(args.inner):
            gb.launch()

    direct()
    torch.cuda.synchronize()
    # the same launches captured once and replayed: no host work between them (and the launch is graph-capturable)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        direct()
    graph.replay()
    torch.cuda.synchronize()
    return gb.grads[0].shape[-1], stream_us(direct), stream_us(graph.replay)


runs = [measure(1), measure(8)]
moved = B * A * (NC * 2 + (64 + NC) * 2) + n_fg * 64 * 2 + B * A * 12  # class logits, gradients, fg box logits, assignment
dense_floor = B * A * (64 + NC) * (2 + 2)

lines = [f"{_lib.version()}; {B} x {SHAPES} x {64 + NC} fp16 level maps, {LABELS} labels per image, {n_fg} foreground "
         f"anchors of {B * A}; {args.reps} repetitions, legs alternated in one process, host wall ms to the synchronise"]
for name, _, _ in legs:
    t = times[name]
    lines.append(f"{name:28}: median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}")
lines.append("the eager leg is fed the device's assignment: it leaves out the TaskAlignedAssigner and so UNDERSTATES the "
             "torch criterion a trainer runs (the reference itself is not measured here)")
for pitch, per_direct, per_graph in runs:
    lines.append(f"ydbl_detect_loss_grad alone, gradient pitch {pitch}, {args.inner} launches between two events, us per "
                 f"launch: replayed from one captured graph median {per_graph[0]:.1f}  min {per_graph[1]:.1f}  max "
                 f"{per_graph[2]:.1f}; enqueued from Python median {per_direct[0]:.1f}  min {per_direct[1]:.1f}  max "
                 f"{per_direct[2]:.1f} (the host's launch rate where it is the larger)")
us = runs[0][2][0]
lines.append(f"  bytes it moves {moved / 1e6:.1f} MB = {moved / HBM * 1e6:.1f} us at {HBM / 1e12:.1f} TB/s "
             f"({moved / (us * 1e-6) / 1e12:.2f} TB/s achieved at pitch {runs[0][0]}); with every logit read and "
             f"written, {dense_floor / 1e6:.1f} MB = {dense_floor / HBM * 1e6:.1f} us")
print("\n".join(lines))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
