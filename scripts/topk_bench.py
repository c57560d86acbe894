"""ydbl_detect_topk alone, next to ydbl_nms on the same candidate lists, alternated in ONE process.

    python scripts/topk_bench.py [--batch 32] [--imgsz 640] [--nc 80] [--rounds 5] [--calls 50]

Candidate lists as the end2end decode writes them in multi-label mode (cap = A * nc per image, cand_idx =
anchor * nc + cls, list order shuffled) from synthetic scores sigmoid(N(-6, 2)) -- no trained YOLOv10 weights exist in
the tree -- cut at conf 0.25, at conf 0.001 and not at all.  Per threshold: the per-image candidate counts, then
`rounds` alternating rounds of `calls` event-timed calls of each kernel (3 untimed calls first: the other kernel's
buffers leave the caches).  ydbl_detect_topk runs the schedule a session would pick (per_image from conf >= 0.1) and,
for comparison, the other one.  Figures, not claims.
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "yolo-dbl_amd"))

import torch  # noqa: E402


def timed(fn, calls):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--nc", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    from ydbl import _lib

    dev = torch.device("cuda")
    B, nc = a.batch, a.nc
    A = sum((a.imgsz // s) ** 2 for s in (8, 16, 32))
    cap = A * nc
    g = torch.Generator(device=dev).manual_seed(0)
    scores = torch.sigmoid(torch.randn(B, cap, generator=g, device=dev) * 2 - 6)
    xy = torch.rand(B, cap, 2, generator=g, device=dev) * a.imgsz
    boxes_all = torch.cat([xy, xy + torch.rand(B, cap, 2, generator=g, device=dev) * 100], 2)
    cb = torch.empty(B, cap, 4, device=dev)
    cs = torch.empty(B, cap, device=dev)
    cc = torch.empty(B, cap, dtype=torch.int32, device=dev)
    ci = torch.empty(B, cap, dtype=torch.int32, device=dev)
    cn = torch.zeros(B, dtype=torch.int32, device=dev)
    out = torch.zeros(B, 300, 6, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    nws = int(_lib.lib.ydbl_detect_topk_workspace(B, cap))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    nms_ws = torch.zeros(int(_lib.lib.ydbl_nms_workspace(B, cap, 30000)), dtype=torch.uint8, device=dev)
    print(f"bs{B} {a.imgsz}^2 nc {nc}: A {A}, cap {cap}; topk workspace {nws / 1e6:.1f} MB, nms workspace "
          f"{nms_ws.numel() / 1e6:.1f} MB")
    for conf in (0.25, 0.001, -1.0):
        for b in range(B):  # the image's list: its candidates in a shuffled order
            idx = torch.nonzero(scores[b] > conf).flatten()
            idx = idx[torch.randperm(len(idx), generator=g, device=dev)]
            n = len(idx)
            cb[b, :n], cs[b, :n], ci[b, :n], cc[b, :n], cn[b] = boxes_all[b, idx], scores[b, idx], idx.int(), (
                idx % nc).int(), n
        counts = cn.tolist()
        stream = torch.cuda.current_stream(dev).cuda_stream

        def topk(per_image):
            d = _lib.TopkDesc(cb.data_ptr(), cs.data_ptr(), cc.data_ptr(), ci.data_ptr(), cn.data_ptr(), B, cap, 300,
                              300, None, 0, float(a.imgsz), float(a.imgsz), out.data_ptr(), cnt.data_ptr(), 0, 0,
                              ws.data_ptr(), nws, per_image)
            return lambda: _lib.check(_lib.lib.ydbl_detect_topk(C.byref(d), stream), "ydbl_detect_topk")

        nd = _lib.NmsDesc(cb.data_ptr(), cs.data_ptr(), cc.data_ptr(), ci.data_ptr(), cn.data_ptr(), B, cap, 0.7, 300,
                          30000, 0, 7680.0, float(a.imgsz), float(a.imgsz), out.data_ptr(), cnt.data_ptr(),
                          nms_ws.data_ptr(), 0, 0, int(conf >= 0.1))
        legs = {"topk per_image": topk(1), "topk split": topk(0),
                "nms": lambda: _lib.check(_lib.lib.ydbl_nms(C.byref(nd), stream), "ydbl_nms")}
        res = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                res[k].append(timed(fn, a.calls if conf > 0 else max(a.calls // 5, 3)))
        print(f"conf {conf if conf > 0 else 'none'}: candidates per image min {min(counts)} median "
              f"{sorted(counts)[B // 2]} max {max(counts)}; session schedule: "
              f"{'per_image' if conf >= 0.1 else 'split'}")
        for k, v in res.items():
            v = sorted(v)
            print(f"  {k:15s} us per call median {v[len(v) // 2]:9.1f}  best {v[0]:9.1f}  all "
                  f"{' '.join(f'{u:.1f}' for u in v)}", flush=True)


if __name__ == "__main__":
    main()
