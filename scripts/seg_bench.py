"""Throughput of yolo11n-seg next to yolo11n on the bench workload, in ONE process in alternating rounds (as
scripts/baseline_bench.py), and the two kernels segmentation adds, alone.

    python scripts/seg_bench.py [--batch 32] [--imgsz 640] [--rounds 5] [--steps 40] [--dets 10]

Legs: yolo11n-seg and yolo11n (tests/golden/*.json layer tables, nc 3, weights seeded: torch.manual_seed(0) +
trained_like_), each model.session(batch, imgsz, imgsz, half=True, streams=2): the two-branch session bench.py
measures.  The segmentation leg's step is the captured graph -- forward, Proto, the coefficient branch, decode, NMS with
out_idx -- without the mask launch, which follows a host read of the counts and is timed on its own below.

Then, from sub-batch plan 0 of yolo11n-seg (batch / 2 images): the in-graph time of the deconv2x2 launch
(Plan.run_graph_timed) against the bytes it moves; and ydbl_process_mask alone over the session's own prototype and
coefficient buffers with --dets synthetic detections per image of the whole batch (boxes of 80..320 pixels a side,
random anchors), one launch per sub-batch plan as predict() issues them, for fp32 and uint8 output, timed with events:
the bytes written and the resulting rate.  Figures, not claims."""
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
    m = YOLO(str(ROOT / "tests" / "golden" / f"{name}.json"), nc=3)
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


def deconv_alone(sess):
    plan = sess.plans[0]
    for st, (what, ms) in zip(plan.steps, plan.run_graph_timed()):
        if what == "deconv2x2":
            x, y = st.args[0].x, st.args[0].y
            b = (x.n * x.h * x.w * x.c + y.n * y.h * y.w * y.c) * 2 + 4 * x.c * y.c * 2
            fl = 2.0 * x.n * x.h * x.w * x.c * 4 * y.c
            print(f"deconv2x2 {x.n}x{x.h}x{x.w}x{x.c} -> {y.n}x{y.h}x{y.w}x{y.c} fp16: {ms * 1e3:.2f} us in graph, "
                  f"{b / 1e6:.1f} MB algorithmic, {b / (ms * 1e-3) / 1e9:.0f} GB/s, "
                  f"{fl / (ms * 1e-3) / 1e12:.2f} TFLOP/s")


def masks_alone(sess, dets, calls):
    from ydbl.utils.ops import launch_process_mask

    B, h, w, dev = sess.batch, sess.h, sess.w, sess.device
    g = torch.Generator().manual_seed(0)
    side = torch.rand(B, dets, 2, generator=g) * 240 + 80
    ctr = torch.rand(B, dets, 2, generator=g) * torch.tensor([float(w), float(h)])
    det = torch.zeros(B, dets, 6)
    det[..., :2] = (ctr - side / 2).clamp(min=0)
    det[..., 2:4] = torch.minimum(ctr + side / 2, torch.tensor([float(w), float(h)]))
    det = det.to(dev)
    keep = torch.randint(0, sess.A, (B, dets), generator=g).int().to(dev)
    cnt = torch.full((B,), dets, dtype=torch.int32, device=dev)
    row = (torch.arange(B, dtype=torch.int64) * dets).to(dev)
    for dtype, name in ((torch.float32, "fp32"), (torch.uint8, "uint8")):
        out = torch.empty((B * dets, h, w), dtype=dtype, device=dev)

        def run():
            for part, (a, b) in zip(sess.parts, sess.bounds):
                pv, mcv = sess._mask_views(part)
                launch_process_mask(pv, det[a:b], cnt[a:b], row[a:b], out, (h, w), window=(0, 0, pv.h, pv.w),
                                    sx=pv.w / w, sy=pv.h / h, crop_after=False, max_det=dets, keep_idx=keep[a:b],
                                    mc=mcv, slots=dets)

        ms = events_ms(run, calls)
        nbytes = out.numel() * out.element_size()
        print(f"ydbl_process_mask {B} images x {dets} detections -> {h}x{w} {name}: {ms * 1e3:.1f} us per batch "
              f"({len(sess.parts)} launches), {nbytes / 1e6:.1f} MB written, {nbytes / (ms * 1e-3) / 1e12:.2f} TB/s; "
              f"ones {out.float().mean().item():.3f} of the pixels")
        del out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--dets", type=int, default=10)
    a = ap.parse_args()
    from ydbl.utils.synthetic import blob_images

    x = blob_images(a.batch, a.imgsz, seed=1234).cuda()
    sess = {}
    for name in ("yolo11n-seg", "yolo11n"):
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
    print(f"bs{a.batch} {a.imgsz}^2 fp16, two-branch session, nc 3, {a.rounds} alternating rounds of {a.steps} steps")
    for name, v in res.items():
        v = sorted(v)
        n = sum(len(p.steps) for p in sess[name].plans)
        med = v[len(v) // 2]
        print(f"{name:12s} launches {n:4d}  img/s median {a.batch / med:9.1f}  ms_per_step median {med * 1e3:7.3f}  "
              f"best {v[0] * 1e3:7.3f}  all {' '.join(f'{u * 1e3:.3f}' for u in v)}", flush=True)
    deconv_alone(sess["yolo11n-seg"])
    masks_alone(sess["yolo11n-seg"], a.dets, 20)


if __name__ == "__main__":
    main()
