"""What coco_eval costs val(): wall time of val() on the workload of scripts/confusion_val_timing.py (DBL-n with the
synthetic weights, in-memory batches of four 128 x 128 images, labels = the model's own conf-0.25 detections) with
coco_eval=True (TP matrix + confusion matrix + COCO matching per batch, COCO accumulate on the host) and
coco_eval=False, in one process and alternating, plus ydbl_coco_match alone on one batch's tensors (HIP events).

--tree PATH imports the package from another checkout (its yolo-dbl_amd/), so the same script times a tree without
the feature: val() there ignores coco_eval and its two rows are the same measurement twice — the run-to-run spread
the coco_eval=False row of this tree is compared with.

    python scripts/coco_val_timing.py [--tree PATH] [--batches 8] [--reps 20] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(ROOT))
ap.add_argument("--batches", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, str(Path(args.tree) / "yolo-dbl_amd"))

import torch  # noqa: E402

from ydbl import YOLO, _lib  # noqa: E402
from ydbl.engine import validator  # noqa: E402
from ydbl.utils.synthetic import blob_images, load_trained  # noqa: E402

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
has_coco = hasattr(validator, "coco_batch")


def run(coco):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = model.val(data=batches, coco_eval=coco)
    m.confusion_matrix.matrix  # the read-back belongs to the cost
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for c in (True, False, True, False):  # compile + warm
    run(c)
times = {True: [], False: []}
for _ in range(args.reps):
    for c in (True, False):
        times[c].append(run(c))
lines = [f"{_lib.version()}; package from {'this tree' if Path(args.tree) == ROOT else 'another tree (--tree)'}; "
         f"val() on {args.batches} in-memory batches of {B} x 3 x {S} x {S} (DBL-n, fp32, conf 0.001, {n_gt} labels), "
         f"{args.reps} alternating repetitions, wall ms per val() call (host metrics included)"
         + ("" if has_coco else "; val() ignores coco_eval here: both rows are the same measurement")]
for c in (True, False):
    t = times[c]
    lines.append(f"coco_eval={c!s:5}: median {statistics.median(t):8.3f}  min {min(t):8.3f}  max {max(t):8.3f}  "
                 f"= {statistics.median(t) / args.batches:.3f} ms per batch")
d = statistics.median(times[True]) - statistics.median(times[False])
lines.append(f"coco_eval=True - coco_eval=False (medians): {d:+.3f} ms per val() = {d / args.batches * 1e3:+.1f} us "
             "per batch")

if has_coco:
    from ydbl.utils.metrics import coco_accumulate

    sess = model.session(B, S, S, conf=0.001, iou=0.7, max_det=300, multi_label=True, device=dev, clip=True)
    det, cnt = sess(x[:B].to(dev))
    det, cnt = det.clone(), cnt.clone()
    b0 = batches[0]
    grouped = validator.group_labels(b0["bboxes"], b0["cls"], b0["batch_idx"], B, dev)
    fn = lambda: validator.coco_batch(det, cnt, None, None, None, 3, grouped=grouped)  # noqa: E731
    out = fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(50):
        fn()
    b.record()
    torch.cuda.synchronize()
    lines.append(f"ydbl_coco_match through its Python launcher (allocations included), one batch, {int(cnt.sum())} "
                 f"detections / {len(b0['cls'])} labels: {a.elapsed_time(b) / 50 * 1e3:.1f} us per call")
    by_image = torch.argsort(b0["batch_idx"].long(), stable=True)
    rec = validator.coco_host_record(det.cpu(), {k: v.cpu() for k, v in out.items()}, b0["cls"][by_image], 3, False)
    t0 = time.perf_counter()
    for _ in range(10):
        coco_accumulate([rec] * args.batches, 3)
    lines.append(f"coco_accumulate on the host, {args.batches} such batches: "
                 f"{(time.perf_counter() - t0) / 10 * 1e3:.3f} ms per call")
print("\n".join(lines))
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
