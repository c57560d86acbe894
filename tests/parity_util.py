"""Shared helpers for the end-to-end parity tests (test infrastructure; imports oracle/).

The oracle restatement (oracle/model.py) is run in three precisions on the same
state_dict and the same input:
- fp64: the BN-folded fp32 weights evaluated in double precision = the "exact"
  answer of the fused network (the reference fuses BN in fp32 too, U/nn/tasks.py:207-235);
- fp32: the reference's own CPU path (U/engine/predictor.py:116-134, AutoBackend fp32);
- fp16: the reference's half=True path (AutoBackend .half(), U/nn/autobackend.py:145-155)
  evaluated by torch-CPU in float16.
The GPU result of a precision is then judged against the fp64 answer with a bound
taken from how far the reference's own path of that precision lands from it.
"""

from __future__ import annotations

import copy
import time

import torch

from oracle.metrics import box_iou as box_iou_xyxy
from oracle.ops import clip_boxes, non_max_suppression

ROLE_FX = {"n": ("yolov13n_DBL.yaml", "trained_yolov13n_DBL_nc{nc}.npz"),
           "s": ("yolov13s_DBL.yaml", "trained_yolov13s_DBL_nc{nc}.npz"),
           "l": ("yolov13l_DBL2.yaml", "trained_yolov13l_DBL2_nc{nc}.npz"),
           "x": ("yolov13x_DBL2.yaml", "trained_yolov13x_DBL2_nc{nc}.npz")}


def build_pair(scale: str, nc: int, golden_dir):
    """(product YOLO, fused fp32 oracle) with identical weights."""
    from oracle.model import build_model
    from ydbl import YOLO
    from ydbl.utils.synthetic import load_trained

    cfg, fx = ROLE_FX[scale]
    fx = golden_dir / fx.format(nc=nc)
    torch.manual_seed(0)
    p = YOLO(cfg, nc=nc)
    load_trained(p.model, fx)
    torch.manual_seed(0)
    o = build_model(cfg, nc=nc)
    load_trained(o, fx)
    o.fuse()
    return p, o


def oracle_only(scale: str, nc: int, golden_dir):
    """The fused fp32 oracle of a BASELINE model with the trained-like fixture."""
    from oracle.model import build_model
    from ydbl.utils.synthetic import load_trained

    cfg, fx = ROLE_FX[scale]
    torch.manual_seed(0)
    o = build_model(cfg, nc=nc)
    load_trained(o, golden_dir / fx.format(nc=nc))
    return o.fuse()


def fp32_rule(st):
    """(box px, score) tolerance of the fp32 comparison: twice the reference fp32 path's worst deviation
    from the fp64 answer (st = err_stats of that leg) plus a floor of 1e-3 px / 1e-6.  Used for class agreement
    and detection matching (the fixture's det_borderline counts were taken at this tolerance)."""
    return 2 * st["box_max"] + 1e-3, 2 * st["conf_max"] + 1e-6


# fp32 value-bound factors per fixture (max, p99.9): the GPU's deviation from fp64 / the oracle fp32 leg's.  Both paths
# are fp32 and differ in summation order (and expf), so their deviations are of one order but not ordered; the factor
# is 2 except where a pinned layout measured above it (round 5, every layout of tests/test_gpu_e2e.py, max / p99.9):
# n640 1.40 / 1.27, s640 box 2.01 (bs8 as two bs4 graphs) and score 2.07 (bs32) / 1.63, l1280 1.65 / 1.71, x640 (a
# fixture ~50x worse conditioned, not a BASELINE model) 1.66 / 2.26
FP32_FACTOR = {"n": (2.0, 2.0), "s": (2.5, 2.0), "l": (2.0, 2.0), "x": (2.0, 3.0)}
# NMS decisions within the tolerance of flipping, beyond twice the reference fp32 path's own count (a count of rare
# events; measured round 5: s640 bs32 one graph 2, every other fixture / layout 0 beyond the reference's)
FP32_BORDERLINE_EXTRA = {"n": 0, "s": 2, "l": 0, "x": 0}
# fp16: final detections whose NMS decision lies within the fp16 tolerance of flipping ("borderline") may number at
# most the reference half path's own count on the fixture + this margin (round 5 measured, every layout: n640 7-12
# against the half path's 35, s640 45-47 against 58, l1280 17-21 against 18, x640 0 against 0)
FP16_BORDERLINE_EXTRA = {"n": 3, "s": 3, "l": 6, "x": 3}


def fp32_rule_max(st, scale):
    """The value bound of the fp32 comparison: the worst and the p99.9 deviation from fp64 each within FP32_FACTOR
    times the reference fp32 path's own (+ the floor).  Returns (box max, score max, box p99.9, score p99.9)."""
    fm, fp = FP32_FACTOR[scale]
    return (fm * st["box_max"] + 1e-3, fm * st["conf_max"] + 1e-6, fp * st["box_p999"] + 1e-4,
            fp * st["conf_p999"] + 1e-7)


def fp16_rule(st):
    """fp16 tolerance: twice the reference half path's p99.9 deviation from fp64 (its max is dominated by
    a handful of anchors whose 16-bin DFL softmax is nearly flat)."""
    return 2 * st["box_p999"] + 1e-2, 2 * st["conf_p999"] + 1e-4


def load_e2e(golden_dir, name):
    """(y64 [R, 4+nc, A] fp64, meta); meta["y32"] = the oracle's own fp32 answer (y64 + the stored fp16 d32) when
    the fixture carries it."""
    import json

    import numpy as np

    with np.load(golden_dir / f"e2e_{name}.npz", allow_pickle=False) as z:
        if "y64" in z.files:
            y = z["y64"]
        else:  # a fixture above 1 MiB keeps y64 beside it, split by image (tests/golden/make_e2e.py save_e2e)
            y = np.concatenate([np.load(golden_dir / f"e2e_{name}.y64_{i}.npz", allow_pickle=False)["y64"]
                                for i in range(int(z["y64_parts"]))])
        y64 = torch.from_numpy(y).double()
        meta = json.loads(str(z["meta"]))
        if "d32" in z.files:
            meta["y32"] = y64 + torch.from_numpy(z["d32"]).double()
        return y64, meta


def batch_images(meta, batch, streams=1):
    """Indices (into the fixture's full synthetic batch) of a `batch`-image test batch that puts the fixture's
    reference images into EVERY sub-batch graph of a streams-way split session (DetectSession: contiguous
    ydbl.parallel.shard_bounds slices): the reference images are dealt to the sub-batches in order, each group
    at the start of its sub-batch with its last image at the sub-batch's end (where the flattened-pixel kernels
    put their ragged last tile); the other positions take the remaining images in order.  A full batch that
    already has reference images in every sub-batch graph is returned unchanged.  Images are independent through
    the network, so a position change is only a routing change (the kernels' tile / workgroup choice depends on
    the sub-batch size, not on the images)."""
    from ydbl.parallel import shard_bounds

    full, ref = meta["batch_full"], list(meta["ref_images"])
    if batch > full:
        raise ValueError(f"batch {batch} > the fixture's {full}")
    bounds = [shard_bounds(batch, streams, r) for r in range(streams)] if streams > 1 else [(0, batch)]
    if batch == full and all(any(a <= i < b for i in ref) for a, b in bounds):
        return list(range(full))  # the full batch already has reference images in every sub-batch graph
    ref = ref[:batch]
    n = len(bounds)
    groups = [ref[len(ref) * i // n: len(ref) * (i + 1) // n] for i in range(n)]
    pos = [None] * batch
    for (a, b), g in zip(bounds, groups):
        g = g[: b - a]
        if not g:
            continue
        pos[a] = g[0]
        if len(g) > 1:
            pos[b - 1] = g[-1]
        for k, im in enumerate(g[1:-1]):
            pos[a + 1 + k] = im
    placed = {p for p in pos if p is not None}
    fill = iter(i for i in range(full) if i not in placed)
    return [p if p is not None else next(fill) for p in pos]


def direct_report(yg, meta):
    """|gpu - oracle fp32| (max box px, max score) on the reference images: the north_star's direct comparison,
    reported beside the fp64 rule (the oracle's fp32 leg is itself ~1e-2 px from fp64 at these sizes)."""
    y32 = meta.get("y32")
    if y32 is None:
        return None
    d = (yg.double() - y32).abs()
    return {"box_max": d[:, :4].max().item(), "conf_max": d[:, 4:].max().item()}


@torch.inference_mode()
def oracle_legs(o, x, legs=("fp64", "fp32")):
    """Decoded predictions y[B, 4+nc, A] (fp32 tensors) of the oracle in each precision + seconds."""
    out, secs = {}, {}
    for leg in legs:
        t0 = time.perf_counter()
        if leg == "fp32":
            y, _ = o(x)
        elif leg == "fp64":
            y, _ = copy.deepcopy(o).double()(x.double())
        elif leg == "fp16":
            y, _ = copy.deepcopy(o).half()(x.half())
        else:
            raise ValueError(leg)
        out[leg] = y.float() if leg != "fp64" else y
        secs[leg] = time.perf_counter() - t0
    return out, secs


def err_stats(y, y64):
    """max / p99.9 abs deviation of boxes (px) and scores from the fp64 answer."""
    y = y.double()
    db = (y[:, :4] - y64[:, :4]).abs().flatten()
    dc = (y[:, 4:] - y64[:, 4:]).abs().flatten()
    q = lambda t: torch.quantile(t[torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:1 << 20]],
                                 0.999).item()
    return {"box_max": db.max().item(), "box_p999": q(db), "conf_max": dc.max().item(), "conf_p999": q(dc)}


def class_agreement(y_gpu, y64, margin):
    """Anchors whose fp64 top-2 class margin exceeds `margin` must have the same argmax class on the GPU
    (torch.max first-index rule, U/utils/ops.py:274).  Returns (checked anchors, disagreements)."""
    nc = y64.shape[1] - 4
    if nc < 2:
        return 0, 0
    s64 = y64[:, 4:]
    top2 = s64.topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > margin
    a = y_gpu[:, 4:].float().argmax(1)
    b = s64.argmax(1)
    return int(safe.sum()), int(((a != b) & safe).sum())


def detections(y, conf, iou, hw, multi_label=False):
    dets = non_max_suppression(y.float(), conf, iou, multi_label=multi_label)
    for d in dets:
        clip_boxes(d[:, :4], hw)  # predict.py:23-41 postprocess -> scale_boxes -> clip_boxes
    return dets


def _borderline(det, y_ref, conf, iou, tol_box, tol_conf, cut):
    """True when the NMS decision about `det` ([6]) can flip under perturbations of tol_box / tol_conf:
    - its score is within tol_conf of the conf threshold, or of the max_det cut (`cut`: the lowest kept
      score of a full image, U/utils/ops.py:300-301), or
    - an anchor at its box has top-2 class scores within 2*tol_conf (the class can flip, :274), or
    - a same-class candidate of comparable-or-higher score overlaps it with an IoU within the IoU change
      a tol_box move can cause (the torchvision keep decision can flip, :296)."""
    if det[4] <= conf + tol_conf or det[4] <= cut + tol_conf:
        return True
    from oracle.ops import xywh2xyxy

    p = y_ref.float().T  # [A, 4+nc]
    sc, cl = p[:, 4:].max(1)
    boxes_all = xywh2xyxy(p[:, :4].clone())
    if p.shape[1] > 5:
        near = (boxes_all - det[:4]).abs().amax(1) <= tol_box
        top2 = p[near, 4:].topk(2, dim=1).values
        if len(top2) and ((top2[:, 0] - top2[:, 1]) <= 2 * tol_conf).any():
            return True
    keep = (sc > conf - tol_conf) & (cl == det[5].long()) & (sc >= det[4] - 2 * tol_conf)
    if not keep.any():
        return False
    ious = box_iou_xyxy(det[None, :4], boxes_all[keep])[0]
    wh = (det[2:4] - det[0:2]).clamp(min=1.0)
    d_iou = 4.0 * tol_box / wh.min().item() + 1e-3  # first-order IoU change for a tol_box shift
    return bool(((ious - iou).abs() <= d_iou).any())


def match_detections(ref, got, y_ref, conf, iou, tol_box, tol_conf, max_det=300):
    """Compare two per-image detection lists both ways: every detection of one set needs a same-class
    detection in the other within (tol_box px, tol_conf).  An unmatched detection is "borderline" when
    its NMS decision can flip under that perturbation (_borderline on the reference predictions y_ref
    [B, 4+nc, A]); anything else is a mismatch.
    Returns dict(pairs, box_dev, conf_dev, borderline, mismatches=[...])."""
    out = {"pairs": 0, "box_dev": 0.0, "conf_dev": 0.0, "borderline": 0, "mismatches": []}
    for b, (r_i, g_i) in enumerate(zip(ref, got)):
        for a_set, b_set, a_is_ref in ((r_i, g_i, True), (g_i, r_i, False)):
            cut = a_set[:, 4].min().item() if len(a_set) >= max_det else -1.0
            for d in a_set:
                if len(b_set):
                    same = b_set[:, 5] == d[5]
                    dev_b = (b_set[:, :4] - d[:4]).abs().amax(1)
                    dev_c = (b_set[:, 4] - d[4]).abs()
                    ok = same & (dev_b <= tol_box) & (dev_c <= tol_conf)
                    if ok.any():
                        j = torch.where(ok, dev_b, torch.full_like(dev_b, 1e9)).argmin()
                        out["box_dev"] = max(out["box_dev"], dev_b[j].item())
                        out["conf_dev"] = max(out["conf_dev"], dev_c[j].item())
                        out["pairs"] += a_is_ref
                        continue
                if _borderline(d, y_ref[b], conf, iou, tol_box, tol_conf, cut):
                    out["borderline"] += 1
                else:
                    out["mismatches"].append(("ref" if a_is_ref else "got", b, [round(v, 3) for v in d.tolist()]))
    return out


def gpu_pred(p, x, half=False, fp8=False, conf=0.25, iou=0.7, calib=None, streams=1):
    """Decoded predictions + final detections of the product path (HIP through libydbl)."""
    B, _, H, W = x.shape
    s = p.session(B, H, W, half=half, conf=conf, iou=iou, keep_pred=True, use_graph=streams > 1, fp8=fp8,
                  streams=streams)
    if fp8:
        s.calibrate_fp8((calib if calib is not None else x).cuda())
    s(x.cuda())
    torch.cuda.synchronize()
    return s.pred.cpu(), s.results()


@torch.inference_mode()
def fp8_emulated_leg(o, x, plan):
    """What fp8 (BASELINE config 5) does to the reference path on its own: the oracle's fp16 leg (the reference's
    half=True path, evaluated by torch-CPU) with every convolution / linear layer that the GPU `plan` switched to
    e4m3 operands (ydbl.quant.enable_fp8: plan.fp8_switched) replaced by its e4m3 emulation at the GPU's
    calibrated scales: input x -> e4m3(x * qs) / qs, weights per output row -> e4m3(w * sw) / sw with
    sw = 448 / max|w_row|, then the fp32 conv + the bias the GPU plan uses (bias correction included).  The plan's candidates are matched to the oracle's modules
    by their (scale-normalised) weight rows, so merged launches (C3's cv2 + cv1) and folded constants
    (DySample's 0.25) map back to the reference's own layers.  Returns (decoded predictions [B, 4+nc, A] fp32,
    number of oracle layers emulated)."""
    import types

    import torch.nn as nn
    import torch.nn.functional as F

    from ydbl.quant import E4M3_MAX, e4m3_round

    rows, owner, dl = [], [], []  # normalised leading 16 values of every switched candidate row, (qs, cin_pad),
    for ci in plan.fp8_switched:  # and the row's bias correction (ydbl.quant.bias_delta; 0 without)
        d, xv, w32 = plan.fp8_candidates[ci]
        w = w32[:, : d.kh * d.kw * xv.c].double()
        w = w / w.abs().amax(1, keepdim=True).clamp_min(1e-30)
        rows.append(w[:, :16])
        owner += [(float(d.qscale), xv.c)] * w.shape[0]
        dl.append(getattr(plan, "fp8_bias_delta", {}).get(ci, torch.zeros(w.shape[0])).float())
    dl = torch.cat(dl) if dl else None
    if not rows:
        raise ValueError("the plan has no fp8-switched convolutions")
    rows = torch.cat(rows)
    m = copy.deepcopy(o).half()
    n_emulated = 0
    for ref_mod, mod in zip(o.modules(), m.modules()):
        if isinstance(ref_mod, nn.Conv2d) and ref_mod.groups == 1:
            w = ref_mod.weight.detach().double()
            co, ci, kh, kw = w.shape
        elif isinstance(ref_mod, nn.Linear):
            w = ref_mod.weight.detach().double()[:, :, None, None]
            co, ci, kh, kw = w.shape
        else:
            continue
        sig = w[0].permute(1, 2, 0)  # [kh][kw][ci] tap-major, as the plan's weight matrix
        hit = None
        for cin_pad in {c for _, c in owner}:
            if cin_pad < ci:
                continue
            r = F.pad(sig, (0, cin_pad - ci)).reshape(-1)
            r = (r / r.abs().max().clamp_min(1e-30))[:16]
            dev = (rows[:, : len(r)] - r).abs().amax(1)
            j = int(dev.argmin())
            if dev[j] < 1e-5 and owner[j][1] == cin_pad:
                hit = owner[j] + (dl[j: j + co],)
                break
        if hit is None:
            continue
        qs = hit[0]
        w32 = ref_mod.weight.detach().float()
        sw = E4M3_MAX / w32.reshape(co, -1).abs().amax(1).clamp_min(1e-12)
        shape = (-1,) + (1,) * (w32.dim() - 1)
        wq = e4m3_round(w32 * sw.view(shape)) / sw.view(shape)
        b32 = ref_mod.bias.detach().float() if ref_mod.bias is not None else torch.zeros(co)
        b32 = b32 - hit[2]  # the GPU's bias correction of this layer

        def fwd(self, inp, wq=wq, b32=b32, qs=qs, conv=isinstance(ref_mod, nn.Conv2d)):
            xq = e4m3_round(inp.float() * qs) / qs
            y = (F.conv2d(xq, wq, b32, self.stride, self.padding, self.dilation) if conv else F.linear(xq, wq, b32))
            return y.to(inp.dtype)

        mod.forward = types.MethodType(fwd, mod)
        n_emulated += 1
    y, _ = m(x.half())
    return y.float(), n_emulated
