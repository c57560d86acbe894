"""Throughput of the baselines next to DBL-n on the bench workload, in ONE process in alternating rounds (as
scripts/ab_bench.py), and the two kernels the YOLO11 / YOLOv8 baselines add, alone.

    python scripts/baseline_bench.py [--batch 32] [--imgsz 640] [--rounds 5] [--steps 40]

Legs: yolo11n, yolov8n, yolov10n, yolov13n (tests/golden/*.json layer tables, nc 3, weights seeded: torch.manual_seed(0) +
trained_like_) and DBL-n (the bench fixture), each model.session(batch, imgsz, imgsz, half=True, streams=2): the
two-branch session bench.py measures (yolov10n's tail is the end2end decode and ydbl_detect_topk, the others' the
NMS).  Figures, not claims: no host reference run exists to form a ratio.

Then, from sub-batch plan 0 of yolo11n (batch / 2 images): the in-graph time of SPPF.pool5x3 and PSA.attn
(Plan.run_graph_timed) against the bytes each moves, and ydbl_psa_attn alone against eager torch
(matmul / softmax / matmul) on one random qkv tensor of the same shape, both timed with events over 200 calls.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "yolo-dbl_amd"))
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from bench import CFGS  # noqa: E402


def build(name):
    from ydbl import YOLO
    from ydbl.utils.synthetic import load_trained, trained_like_

    torch.manual_seed(0)
    if name == "DBL-n":
        cfg, fx = CFGS["n"]
        m = YOLO(cfg, nc=3)
        load_trained(m.model, ROOT / "tests" / "golden" / fx)
        return m
    m = YOLO(str(ROOT / "tests" / "golden" / f"{name}.json"), nc=3)
    trained_like_(m.model, 0)
    return m


def events_ms(fn, n=200):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def kernels_alone(sess):
    from ydbl import _lib
    from ydbl.runtime import Plan

    plan = sess.plans[0]
    times = plan.run_graph_timed()
    for st, (what, ms) in zip(plan.steps, times):
        if what == "SPPF.pool5x3":
            v = st.args[0].x
            b = 4 * v.n * v.h * v.w * v.c * 2  # x read once, three maps written
            print(f"SPPF.pool5x3 {v.n}x{v.h}x{v.w}x{v.c} fp16: {ms * 1e3:.2f} us in graph, {b / 1e3:.0f} KB algorithmic, "
                  f"{b / (ms * 1e-3) / 1e9:.0f} GB/s")
        if what == "PSA.attn":
            d = st.args[0]
            q = d.qkv
            b = q.n * q.h * q.w * (q.c + 2 * d.y.c) * 2  # qkv read, y and v written
            fl = 2.0 * q.n * d.heads * (q.h * q.w) ** 2 * (32 + 64)
            print(f"PSA.attn {q.n}x{q.h}x{q.w}x{q.c} heads {d.heads} fp16: {ms * 1e3:.2f} us in graph, "
                  f"{b / 1e3:.0f} KB algorithmic, {b / (ms * 1e-3) / 1e9:.0f} GB/s, {fl / (ms * 1e-3) / 1e12:.2f} TFLOP/s")
            n, h, w, heads = q.n, q.h, q.w, d.heads
    p = Plan(torch.device("cuda"), torch.float16)
    qv, y, vv = p.alloc(n, h, w, heads * 128), p.alloc(n, h, w, heads * 64), p.alloc(n, h, w, heads * 64)
    qv.torch().copy_(torch.randn(n, h, w, heads * 128, generator=torch.Generator().manual_seed(0)))
    dd = _lib.PsaAttnDesc(qv.struct(), y.struct(), vv.struct(), heads, 32, 64, 32**-0.5)
    p.launch("ydbl_psa_attn", dd, what="attn", keep=[dd])
    t = qv.torch().reshape(n, h * w, heads, 128).permute(0, 2, 1, 3)  # [n, heads, N, 128] view of the same memory
    qq, kk, vt = t[..., :32], t[..., 32:64], t[..., 64:]

    def eager():
        return (qq @ kk.transpose(-2, -1) * 32**-0.5).softmax(-1) @ vt

    ms_k, ms_e = events_ms(p.run), events_ms(eager)
    err = (eager().permute(0, 2, 1, 3).reshape(n, h, w, heads * 64).float() - y.torch().float()).abs().max().item()
    print(f"ydbl_psa_attn alone {ms_k * 1e3:.2f} us per call, eager torch matmul/softmax/matmul {ms_e * 1e3:.2f} us "
          f"(x{ms_e / ms_k:.1f}); max |difference| {err:.3g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    from ydbl.utils.synthetic import blob_images

    x = blob_images(a.batch, a.imgsz, seed=1234).cuda()
    sess = {}
    for name in ("yolo11n", "yolov8n", "yolov10n", "yolov13n", "DBL-n"):
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
        print(f"{name:9s} launches {n:4d}  img/s median {a.batch / med:9.1f}  ms_per_step median {med * 1e3:7.3f}  "
              f"best {v[0] * 1e3:7.3f}  all {' '.join(f'{u * 1e3:.3f}' for u in v)}", flush=True)
    kernels_alone(sess["yolo11n"])


if __name__ == "__main__":
    main()
