"""A/B of the HIP A2C2f against what a user had before it: the restated torch A2C2f (tests/a2c2f_util.py) registered
as a forward-only plugin, which runs inside the plan as a captured torch step on NCHW views (nn.modules.emit_torch).
Both are one-module plans in ONE process on the same input, each captured into a hipGraph, timed in alternating
repetitions; fp16.  The HIP plan's per-launch times (Plan.run_graph_timed) give the attention launch's share.

    python scripts/a2c2f_ab.py [--rounds 7] [--steps 50] [--timeout 240] [--model]

Shapes: yolov13n layer 6 (128 -> 128, n 2, area 4, 16 x 128 x 40 x 40) and layer 8 (256 -> 256, n 2, area 1,
16 x 256 x 20 x 20).  Each shape runs in a child process of its own under --timeout seconds; a child that fails or
runs out of time ends the script (nothing more is started on the GPU).  --model adds one more child: yolov13n (nc 3,
init weights) as session(32, 640, 640, half=True, streams=2), timed the way bench.py times its step (20 untimed steps,
then 100 between device syncs); alone, it is a figure and no comparison.
"""
import argparse
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = {"layer6": ((128, 128, 2, True, 4), (16, 128, 40, 40)), "layer8": ((256, 256, 2, True, 1), (16, 256, 20, 20))}


def child(name, rounds, steps):
    sys.path[:0] = [str(ROOT / "yolo-dbl_amd"), str(ROOT), str(ROOT / "tests")]
    import torch

    import a2c2f_util as U
    from ydbl.nn import modules as M
    from ydbl.runtime import GraphRunner, Plan
    from ydbl.utils.synthetic import trained_like_

    args, (n, c, h, w) = SHAPES[name]
    torch.manual_seed(0)
    ref = trained_like_(U.A2C2f(*args).eval(), 0)
    hip = M.A2C2f(*args)
    hip.load_state_dict(ref.state_dict(), strict=True)
    x = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(1)).half().cuda()
    plans, outs = {}, {}
    for key, emit in (("hip", lambda p, v: M.emit_module(hip, p, v)), ("plugin", lambda p, v: M.emit_torch(U.fuse_(ref), p, v))):
        p = Plan(torch.device("cuda"), torch.float16)
        v = p.alloc(n, h, w, c)
        v.torch().copy_(x)
        outs[key] = emit(p, v)
        plans[key] = (p, GraphRunner(p, warmup=2))
    torch.cuda.synchronize()
    d = (outs["hip"].torch().float() - outs["plugin"].torch().float()).abs().max().item()
    res = {k: [] for k in plans}
    for _ in range(rounds):
        for k, (_, g) in plans.items():
            for _ in range(3):  # untimed: the other variant's buffers leave the caches first
                g.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                g.replay()
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / steps * 1e6)
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    per = plans["hip"][0].run_graph_timed()
    tot = sum(t for _, t in per)
    att = sum(t for wh, t in per if wh.startswith("AAttn.area"))
    print(f"{name}: A2C2f{args} on {n}x{c}x{h}x{w} fp16, max |hip - plugin| {d:.3g}")
    for k in plans:
        print(f"  {k:7s} launches {len(plans[k][0].steps):3d}  us/forward median {med[k]:8.1f}  all "
              f"{' '.join(f'{u:.1f}' for u in sorted(res[k]))}")
    print(f"  plugin / hip = {med['plugin'] / med['hip']:.2f}x;  attention launches {att * 1e3:.1f} us of "
          f"{tot * 1e3:.1f} us summed kernel time = {100 * att / tot:.1f} %", flush=True)
    by = {}
    for wh, t in per:
        by[wh] = by.get(wh, 0.0) + t
    print("  hip launches: " + ", ".join(f"{wh} {t * 1e3:.1f}" for wh, t in sorted(by.items(), key=lambda kv: -kv[1])))
    return 0 if med["hip"] < med["plugin"] else 3


def whole_model():
    sys.path[:0] = [str(ROOT / "yolo-dbl_amd"), str(ROOT)]
    import torch

    from ydbl import YOLO
    from ydbl.utils.synthetic import blob_images, trained_like_

    torch.manual_seed(0)
    model = YOLO(str(ROOT / "tests" / "golden" / "yolov13n.json"), nc=3)
    trained_like_(model.model, 0)
    s = model.session(32, 640, 640, half=True, conf=0.25, iou=0.7, streams=2)
    s.load(blob_images(32, 640, seed=1234).cuda())
    for _ in range(20):
        s()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(100):
        s()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    print(f"yolov13n nc3 session(32, 640, 640, half=True, streams=2): {el * 10:.3f} ms/step, {3200 / el:.0f} images/s, "
          f"{sum(len(p.steps) for p in s.plans)} launches", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--model", action="store_true")
    a = ap.parse_args()
    if a.child:
        return whole_model() if a.child == "model" else child(a.child, a.rounds, a.steps)
    for name in [*SHAPES, *(["model"] if a.model else [])]:
        r = subprocess.run([sys.executable, __file__, "--child", name, "--rounds", str(a.rounds), "--steps",
                            str(a.steps)], timeout=a.timeout)
        if r.returncode:
            print(f"{name}: exit status {r.returncode}; stopping")
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
