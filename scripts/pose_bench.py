"""Throughput of yolo11n-pose next to yolo11n on the bench workload, in ONE process in alternating rounds (as
scripts/seg_bench.py), and the two launches pose adds, alone.

    python scripts/pose_bench.py [--batch 32] [--imgsz 640] [--rounds 5] [--steps 40] [--labels 10]

Legs: yolo11n-pose (nc 1, kpt_shape [17, 3]) and yolo11n (nc 1), tests/golden/*.json layer tables, weights seeded:
torch.manual_seed(0) + trained_like_; each model.session(batch, imgsz, imgsz, half=True, streams=2): the two-branch
session bench.py measures.  The pose leg's step is the whole captured graph -- forward, the keypoint branch, decode, NMS
with out_idx and ydbl_pose_keypoints -- so it returns boxes and keypoints with no host sync.

Then, from sub-batch plan 0 of yolo11n-pose (batch / 2 images): the in-graph time of the ydbl_pose_keypoints launch
(Plan.run_graph_timed) against the bytes it writes; and ydbl_kpt_oks alone over the session's own kpts / count with
--labels synthetic labels per image, timed with events.  Figures, not claims."""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "yolo-dbl_amd"))
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402


def build(name):
    from ydbl import YOLO
    from ydbl.utils.synthetic import trained_like_

    torch.manual_seed(0)
    m = YOLO(str(ROOT / "tests" / "golden" / f"{name}.json"), nc=1)
    trained_like_(m.model, 0)
    return m


def events_ms(fn, n):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def keypoints_alone(sess):
    plan = sess.plans[0]
    timed = plan.run_graph_timed()
    for st, (what, ms) in zip(plan.steps, timed):
        if what == "Pose.keypoints":
            d = st.args[0]
            out = d.n * d.max_det * d.K * d.ndim * 4
            print(f"ydbl_pose_keypoints {d.n} images x {d.max_det} slots x {d.K} x {d.ndim}: {ms * 1e3:.2f} us in graph, "
                  f"{out / 1e3:.1f} KB written ({d.K * d.ndim * 4} bytes per slot), {out / (ms * 1e-3) / 1e9:.1f} GB/s")
    branch = [ms for what, ms in timed if ".pad" in what or what == "Pose.kpt"]
    print(f"keypoint branch (cv4: {len(branch)} conv launches of plan 0): {sum(branch) * 1e3:.1f} us in graph")


def oks_alone(sess, labels, calls):
    from ydbl.utils.metrics import OKS_SIGMA
    from ydbl.utils.ops import kpt_oks

    B, dev = sess.batch, sess.device
    g = torch.Generator().manual_seed(0)
    n_gt = B * labels
    xy = torch.rand(n_gt, 2, generator=g) * 400
    wh = torch.rand(n_gt, 2, generator=g) * 200 + 40
    box = torch.cat([xy, xy + wh], 1).to(dev)
    gk = torch.cat([xy[:, None] + torch.rand(n_gt, 17, 2, generator=g) * wh[:, None],
                    torch.randint(0, 3, (n_gt, 17, 1), generator=g).float()], -1).to(dev)
    ofs = (torch.arange(B + 1, dtype=torch.int32) * labels).to(dev)
    sigma = torch.tensor(OKS_SIGMA, dtype=torch.float32, device=dev)
    count = torch.full((B,), sess.max_det, dtype=torch.int32, device=dev)  # every slot live: the most work
    ms = events_ms(lambda: kpt_oks(sess.kpts, count, gk, box, ofs, sigma), calls)
    pairs = n_gt * sess.max_det
    print(f"ydbl_kpt_oks {B} images x {labels} labels x {sess.max_det} slots: {ms * 1e3:.1f} us per batch "
          f"(allocation of the [n_gt, max_det] output included), {pairs} pairs, {pairs * 4 / 1e3:.0f} KB written, "
          f"{sess.kpts.numel() * 4 / 1e6:.2f} MB of keypoints read")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--labels", type=int, default=10)
    a = ap.parse_args()
    from ydbl.utils.synthetic import blob_images

    x = blob_images(a.batch, a.imgsz, seed=1234).cuda()
    sess = {}
    for name in ("yolo11n-pose", "yolo11n"):
        s = build(name).session(a.batch, a.imgsz, a.imgsz, half=True, conf=0.25, iou=0.7, streams=2)
        s.load(x)
        for _ in range(5):
            s()
        torch.cuda.synchronize()
        sess[name] = s
    res = {k: [] for k in sess}
    for _ in range(a.rounds):
        for name, s in sess.items():
            for _ in range(3):  # untimed: the previous leg's buffers leave the caches first
                s()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                s()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / a.steps)
    print(f"bs{a.batch} {a.imgsz}^2 fp16, two-branch session, nc 1, {a.rounds} alternating rounds of {a.steps} steps")
    for name, v in res.items():
        v = sorted(v)
        n = sum(len(p.steps) for p in sess[name].plans)
        med = v[len(v) // 2]
        print(f"{name:12s} launches {n:4d}  img/s median {a.batch / med:9.1f}  ms_per_step median {med * 1e3:7.3f}  "
              f"best {v[0] * 1e3:7.3f}  all {' '.join(f'{u * 1e3:.3f}' for u in v)}", flush=True)
    print(f"detections of the timed batch: {sess['yolo11n-pose'].count.sum().item()} (seeded weights)")
    keypoints_alone(sess["yolo11n-pose"])
    oks_alone(sess["yolo11n-pose"], a.labels, 20)


if __name__ == "__main__":
    main()
