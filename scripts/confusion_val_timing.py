"""What the confusion-matrix launch costs val(): wall time of val() on the tensor-batch test workload (DBL-n with
the synthetic weights, in-memory batches of four 128 x 128 images, labels = the model's own conf-0.25 detections)
with plots=True (TP matrix + confusion matrix, one launch each per batch) and plots=False (TP matrix only), in one
process and alternating, plus the two launches alone on one batch's tensors (HIP events).

The script also runs on a tree without the feature (val() there ignores plots): its two columns are then the same
measurement twice, which gives the plots=False column of this tree something to be compared with.

    python scripts/confusion_val_timing.py [--batches 8] [--reps 20] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "yolo-dbl_amd"))
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from ydbl import YOLO, _lib  # noqa: E402
from ydbl.engine import validator  # noqa: E402
from ydbl.utils.synthetic import blob_images, load_trained  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

B, S = 4, 128
torch.manual_seed(0)
model = YOLO("yolov13n_DBL.yaml", nc=3)
load_trained(model.model, ROOT / "tests" / "golden" / "trained_yolov13n_DBL_nc3.npz")
dev = torch.device("cuda", 0)
x = blob_images(B * args.batches, S, seed=77)
gt = model.session(B, S, S, conf=0.25, iou=0.7, max_det=300, device=dev)
batches = []
for i in range(0, len(x), B):
    det, cnt = (t.cpu() for t in gt(x[i:i + B].to(dev)))
    rows = [det[j, : int(cnt[j])] for j in range(B)]
    batches.append({"img": x[i:i + B], "cls": torch.cat([r[:, 5] for r in rows]),
                    "bboxes": torch.cat([r[:, :4] for r in rows]),
                    "batch_idx": torch.cat([torch.full((len(r),), j) for j, r in enumerate(rows)])})
n_gt = sum(len(b["cls"]) for b in batches)


def run(plots):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = model.val(data=batches, plots=plots)
    if getattr(m, "confusion_matrix", None) is not None:
        m.confusion_matrix.matrix  # the read-back belongs to the cost
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for p in (True, False, True, False):  # compile + warm
    run(p)
times = {True: [], False: []}
for _ in range(args.reps):
    for p in (True, False):
        times[p].append(run(p))
lines = [f"{_lib.version()}; val() on {args.batches} in-memory batches of {B} x 3 x {S} x {S} (DBL-n, fp32, conf 0.001, "
         f"{n_gt} labels), {args.reps} alternating repetitions, wall ms per val() call (host metrics included)"]
for p in (True, False):
    t = times[p]
    lines.append(f"plots={p!s:5}: median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}  "
                 f"= {statistics.median(t) / args.batches:.3f} ms per batch")
d = statistics.median(times[True]) - statistics.median(times[False])
lines.append(f"plots=True - plots=False (medians): {d:+.3f} ms per val() = {d / args.batches * 1e3:+.1f} us per batch")

if hasattr(validator, "confusion_batch"):
    from ydbl.utils.metrics import ConfusionMatrix

    sess = model.session(B, S, S, conf=0.001, iou=0.7, max_det=300, multi_label=True, device=dev, clip=True)
    det, cnt = sess(x[:B].to(dev))
    det, cnt = det.clone(), cnt.clone()
    b0 = batches[0]
    grouped = validator.group_labels(b0["bboxes"], b0["cls"], b0["batch_idx"], B, dev)
    cm = ConfusionMatrix(3)
    calls = {"ydbl_match_predictions": lambda: validator.match_batch(det, cnt, None, None, None, grouped=grouped),
             "ydbl_confusion_matrix": lambda: validator.confusion_batch(det, cnt, None, None, None, cm, grouped=grouped)}
    for name, fn in calls.items():
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(50):
            fn()
        b.record()
        torch.cuda.synchronize()
        lines.append(f"{name} through its Python launcher (allocations included), one batch, {int(cnt.sum())} "
                     f"detections / {len(b0['cls'])} labels: {a.elapsed_time(b) / 50 * 1e3:.1f} us per call")
print("\n".join(lines))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
