"""What loss=True costs val(), and that loss=False costs nothing: wall time of val() on the f1 workload of DESIGN §0
(DBL-n with the synthetic weights, in-memory batches of four 128 x 128 images, fp32, labels = the model's own conf-0.25
detections) with loss=True and loss=False on this tree and, with --parent PATH (a built checkout of the parent
commit), on that tree too -- all in ONE process, alternating parent / this / parent / this per repetition, so the
rows share the machine's state.  The two packages live side by side: each keeps its own ``ydbl`` modules (swapped
into sys.modules around its calls) and its own libydbl.so.  Plus the loss launch's own time from the in-graph
per-launch profile of the loss session (Plan.run_graph_timed).

    python scripts/loss_val_timing.py [--parent PATH] [--batches 8] [--reps 20] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None)
ap.add_argument("--batches", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch  # noqa: E402

B, S = 4, 128


def _ours():
    return [k for k in sys.modules if k == "ydbl" or k.startswith("ydbl.")]


class Tree:
    """One checkout's ``ydbl`` package: inside ``with tree:`` its modules are the ones sys.modules knows."""

    def __init__(self, root):
        self.root, self.path, self.mods = Path(root), str(Path(root) / "yolo-dbl_amd"), {}
        with self:
            from ydbl import YOLO, _lib
            from ydbl.utils.synthetic import blob_images, load_trained

            self.version = _lib.version()
            torch.manual_seed(0)
            self.model = YOLO("yolov13n_DBL.yaml", nc=3)
            load_trained(self.model.model, ROOT / "tests" / "golden" / "trained_yolov13n_DBL_nc3.npz")
            self.blob_images = blob_images
            import inspect

            self.has_loss = "loss" in inspect.signature(self.model.val).parameters

    def __enter__(self):
        self._saved = {k: sys.modules.pop(k) for k in _ours()}
        sys.modules.update(self.mods)
        sys.path.insert(0, self.path)
        return self

    def __exit__(self, *exc):
        sys.path.remove(self.path)
        self.mods = {k: sys.modules.pop(k) for k in _ours()}
        sys.modules.update(self._saved)

    def val(self, batches, loss):
        with self:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = self.model.val(data=batches, **({"loss": True} if loss else {}))
            m.confusion_matrix.matrix  # the read-back belongs to the cost
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3


this = Tree(ROOT)
parent = Tree(args.parent) if args.parent else None
dev = torch.device("cuda", 0)
x = this.blob_images(B * args.batches, S, seed=77)
with this:
    gt = this.model.session(B, S, S, conf=0.25, iou=0.7, max_det=300, device=dev)
    batches = []
    for i in range(0, len(x), B):
        det, cnt = (t.cpu() for t in gt(x[i:i + B].to(dev)))
        rows = [det[j, : int(cnt[j])] for j in range(B)]
        batches.append({"img": x[i:i + B], "cls": torch.cat([r[:, 5] for r in rows]),
                        "bboxes": torch.cat([r[:, :4] for r in rows]),
                        "batch_idx": torch.cat([torch.full((len(r),), j) for j, r in enumerate(rows)])})
n_gt = sum(len(b["cls"]) for b in batches)

legs = [("this loss=False", this, False), ("this loss=True", this, True)]
if parent:  # parent / this / parent / this; the parent's two legs are the same measurement twice: its own spread
    legs = [("parent", parent, False), ("this loss=False", this, False), ("parent (again)", parent, False),
            ("this loss=True", this, True)]
for _ in range(2):  # compile + warm
    for _, tree, loss in legs:
        tree.val(batches, loss)
times = {name: [] for name, _, _ in legs}
for r in range(args.reps):  # the cycle starts one leg later each repetition: no leg always follows the same one's state
    k = r % len(legs)
    for name, tree, loss in legs[k:] + legs[:k]:
        times[name].append(tree.val(batches, loss))

lines = [f"{this.version}; val() on {args.batches} in-memory batches of {B} x 3 x {S} x {S} (DBL-n, fp32, conf 0.001, "
         f"{n_gt} labels), {args.reps} repetitions of {' / '.join(n for n, _, _ in legs)} in one process, wall ms per "
         f"val() call (host metrics included)"]
if parent:
    lines.append(f"parent: {parent.version} from another checkout" + ("" if not parent.has_loss else " (it has loss=!)"))
for name, _, _ in legs:
    t = times[name]
    lines.append(f"{name:16}: median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}  "
                 f"= {statistics.median(t) / args.batches:.3f} ms per batch")
med = {n: statistics.median(t) for n, t in times.items()}
d = med["this loss=True"] - med["this loss=False"]
lines.append(f"loss=True - loss=False (medians): {d:+.3f} ms per val() = {d / args.batches * 1e3:+.1f} us per batch")
if parent:
    lines.append(f"this loss=False - parent (medians): {med['this loss=False'] - med['parent']:+.3f} ms; the parent's two "
                 f"legs differ by {med['parent (again)'] - med['parent']:+.3f} ms (its own spread)")

with this:
    sess = this.model.session(B, S, S, conf=0.001, iou=0.7, max_det=300, multi_label=True, device=dev, clip=True,
                              use_graph=False, loss=True)
    from ydbl.utils.loss import pad_targets

    b0 = batches[0]
    sess.load_labels(pad_targets(b0["batch_idx"], b0["cls"], b0["bboxes"], B, None, sess.loss.max_labels, xywh=False))
    sess.load(b0["img"].to(dev))
    prof = sess.plan.run_graph_timed()
    total = sum(ms for _, ms in prof)
    own = sum(ms for what, ms in prof if what == "Detect.loss")
    lines.append(f"in-graph per-launch profile of the loss session (batch {B}, {len(b0['cls'])} labels, max_labels "
                 f"{sess.loss.max_labels}): Detect.loss (its five kernels) {own * 1e3:.1f} us of {total * 1e3:.1f} us "
                 f"over {len(prof)} launches")
print("\n".join(lines))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
