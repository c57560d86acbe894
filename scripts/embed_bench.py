"""embed() against the full forward on the bench workload, in ONE process in alternating rounds (as scripts/ab_bench.py),
and the pool kernel's own in-graph time (Plan.run_graph_timed, as scripts/layer_profile.py).

    python scripts/embed_bench.py [--model n] [--batch 32] [--imgsz 640] [--embed 34] [--rounds 5] [--steps 40]

A: model.session(batch, imgsz, imgsz, half=True, embed=[...], streams=default_streams(batch))   the embed session
B: model.session(batch, imgsz, imgsz, half=True, nms=False, streams=2)                          forward + decode
The embed plan is a prefix of B's launches plus one pool per sub-batch plan.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="n")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--embed", type=int, nargs="+", default=[34])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    a = ap.parse_args()
    from ydbl import YOLO
    from ydbl.engine.session import default_streams
    from ydbl.utils.synthetic import blob_images, load_trained

    cfg, fx = CFGS[a.model]
    torch.manual_seed(0)
    model = YOLO(cfg, nc=3)
    load_trained(model.model, ROOT / "tests" / "golden" / fx)
    x = blob_images(a.batch, a.imgsz, seed=1234).cuda()
    sess = {
        "embed": model.session(a.batch, a.imgsz, a.imgsz, half=True, embed=a.embed, streams=default_streams(a.batch)),
        "forward": model.session(a.batch, a.imgsz, a.imgsz, half=True, nms=False, streams=2),
    }
    for s in sess.values():
        s.load(x)
        for _ in range(5):
            s.launch()
    torch.cuda.synchronize()
    res = {k: [] for k in sess}
    for _ in range(a.rounds):
        for name, s in sess.items():
            for _ in range(3):  # untimed: the other session's buffers leave the caches first
                s.launch()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                s.launch()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    print(f"DBL-{a.model} bs{a.batch} {a.imgsz}^2 fp16, embed={a.embed}, {a.rounds} alternating rounds of {a.steps} steps")
    for name, v in res.items():
        v = sorted(v)
        n = sum(len(p.steps) for p in sess[name].plans)
        print(f"{name:8s} launches {n:4d}  ms_per_step median {v[len(v) // 2]:7.4f}  best {v[0]:7.4f}  "
              f"all {' '.join(f'{u:.4f}' for u in v)}", flush=True)
    # the pool launches of one sub-batch plan, timed inside a graph of their own
    plan = sess["embed"].plans[0]
    times = plan.run_graph_timed()
    total = sum(ms for _, ms in times)
    print(f"sub-batch plan 0: {len(times)} launches, in-graph sum {total * 1e3:.1f} us")
    for st, (what, ms) in zip(plan.steps, times):
        if what == "embed.pool":
            d = st.args[0]
            el = 2 if d.x.dtype == 1 else 4
            b = d.x.n * d.x.h * d.x.w * d.x.c * el
            print(f"embed.pool {d.x.n}x{d.x.h}x{d.x.w}x{d.x.c} (cs {d.x.cs}): {ms * 1e3:.2f} us, {b / 1e3:.0f} KB read, "
                  f"{b / (ms * 1e-3) / 1e9:.0f} GB/s, workspace {d.workspace_bytes} B")


if __name__ == "__main__":
    main()
