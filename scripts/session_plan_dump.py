"""Fingerprint of the launch plans of a fixed matrix of sessions, as JSON: what a refactor of the session classes must
leave untouched.  DBL-n nc 3 at 96 x 128 (the smallest input with three valid levels; P5 is 3 x 4), batch 2:

    python scripts/session_plan_dump.py                      # the meta device: tests/golden/session_plans_meta.json
    python scripts/session_plan_dump.py --device cuda --split --fp8 tests/golden/fp8_calib_yolov13s_DBL_nc3.json

Per plan: the ordered (entry point, what) list and, for every ctypes descriptor argument, each view's (n, h, w, c,
cs, dtype) and every scalar field -- in full for the launches a session adds behind the forward (decode, NMS, loss,
scale_img, embed pool), and as ONE digest per plan over the records of all its launches (--full prints every record
instead, to find a difference).  The (entry point, what) pairs are numbered in a table shared by all plans.
Addresses are reduced to null / non-null, except the outputs and candidate lists of the decode, NMS, scale_img and
embed-pool descriptors: those are byte offsets from the session's det / count / pred / out (a split session's shared
ones), the plan owner's cand_* tensors and its staging buffer -- which shows that a sub-batch plan writes its rows of
the shared outputs.  (On the meta device an address is the tensor's byte offset in its storage, so a storage's start
is null there: no launch is fused, and the offsets still show the rows.)  --split adds the batch 5, streams=2 forms;
--fp8 one DBL-s fp8=0.1 session with that calibration.  One line per session.

--list heads: the second matrix (HEADS) instead, an end2end head (tests/golden/yolov10.json: decode_e2e + top-k) and a
Segment head (tests/golden/yolo11-seg.json: the NMS also writes keep_idx), both scale n, nc 3, fp16 at the same size:
tests/golden/session_plans_heads_meta.json.  --list all: both matrices in one file.

The script uses only the public constructors with keywords, ``children``, ``plans`` and ``plan.steps``.
"""
import argparse
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "yolo-dbl_amd")]

import torch  # noqa: E402

from ydbl import YOLO  # noqa: E402
from ydbl.engine.session import AugmentSession, DetectSession, EmbedSession  # noqa: E402

H, W = 96, 128
CAND = ("cand_box", "cand_score", "cand_cls", "cand_idx", "cand_count")
# entry point -> {descriptor field: (holder, attribute)}: the tensor an address is written relative to
RELATIVE = {
    "ydbl_detect_decode": {"y_ref": ("top", "pred"), **{f: ("own", f) for f in CAND}},
    "ydbl_detect_decode_aug": {"y_ref": ("top", "pred"), **{f: ("own", f) for f in CAND}},
    "ydbl_detect_decode_e2e": {"y_ref": ("top", "pred"), **{f: ("own", f) for f in CAND}},
    "ydbl_nms": {"out": ("top", "det"), "out_count": ("top", "count"), "out_idx": ("own", "keep_idx"),
                 **{f: ("own", f) for f in CAND}},
    "ydbl_detect_topk": {"out": ("top", "det"), "out_count": ("top", "count"), **{f: ("own", f) for f in CAND}},
    "ydbl_scale_img": {"x": ("own", "input")},
    "ydbl_global_avgpool": {"y": ("top", "out")},
}
TAIL = (*RELATIVE, "ydbl_detect_loss")
VARIANTS = [
    ("detect_fp16", DetectSession, dict(dtype=torch.float16, conf=0.25)),
    ("detect_fp16_val", DetectSession, dict(dtype=torch.float16, conf=0.001, multi_label=True)),
    ("detect_fp32", DetectSession, dict(dtype=torch.float32)),
    ("detect_pred_no_nms", DetectSession, dict(dtype=torch.float16, keep_pred=True, nms=False)),
    ("detect_classes", DetectSession, dict(dtype=torch.float16, classes=[0, 2])),
    ("detect_no_clip", DetectSession, dict(dtype=torch.float16, clip=False)),
    ("detect_gather_rows", DetectSession, dict(dtype=torch.float16, gather_rows=3)),
    ("detect_loss", DetectSession, dict(dtype=torch.float16, loss={"max_labels": 8})),
    ("augment", AugmentSession, dict(dtype=torch.float16)),
    ("augment_pred", AugmentSession, dict(dtype=torch.float16, keep_pred=True)),
    ("embed", EmbedSession, dict(dtype=torch.float16, embed=[4, 9])),
]
# the second matrix: (name, model file, session class, settings)
HEADS = [
    ("e2e", "yolov10n.json", DetectSession, dict(dtype=torch.float16)),
    ("e2e_pred_no_nms", "yolov10n.json", DetectSession, dict(dtype=torch.float16, keep_pred=True, nms=False)),
    ("e2e_classes", "yolov10n.json", DetectSession, dict(dtype=torch.float16, classes=[0, 2])),
    ("seg", "yolo11n-seg.json", DetectSession, dict(dtype=torch.float16)),
    ("seg_val", "yolo11n-seg.json", DetectSession, dict(dtype=torch.float16, conf=0.001, multi_label=True)),
]
SPLIT = ("detect_fp16", "detect_fp16_val", "detect_pred_no_nms", "augment", "augment_pred", "embed",
         "e2e", "e2e_pred_no_nms", "seg", "seg_val")


def _addr(v, base):
    if base is not None:  # a field the session always sets: its distance from the tensor it must lie in
        return {"off": int(v or 0) - base.data_ptr()}
    return "addr" if v else None


def _value(v, tp, base=None):
    if tp is C.c_void_p:
        return _addr(v, base)
    if isinstance(v, C.Structure):
        return _struct(v, {})
    if isinstance(v, C.Array):
        return [_value(e, tp._type_) for e in v]
    return v


# Optional descriptor fields appended to the C ABI after the fingerprint was recorded, each documented as "NULL =
# the behaviour before the field existed": left out of a record while unset, so that the recorded plans stay
# comparable; a session that sets one (a segmentation model's NMS writes out_idx: it has a keep_idx, also on the meta
# device, where the address itself is null) shows it.
APPENDED = {"NmsDesc": ("out_idx",)}


def _struct(d, rel):
    late = APPENDED.get(type(d).__name__, ())
    return {name: _value(getattr(d, name), tp, rel.get(name)) for name, tp in d._fields_
            if not (name in late and not getattr(d, name) and rel.get(name) is None)}


def plan_fingerprint(plan, top, own) -> list:
    """One plan's steps, every record in full; `top` holds the det / count / pred the plan writes into, `own` the
    plan's candidate lists."""
    holders = {"top": top, "own": own}
    steps = []
    for st in plan.steps:
        name = st.fn.__name__
        rel = {}
        for f, (who, attr) in RELATIVE.get(name, {}).items():
            h = holders[who]
            rel[f] = h.compiled.input if attr == "input" else getattr(h, attr, None)
        args = []
        for a in st.args:
            if isinstance(a, C.Structure):
                args.append({type(a).__name__: _struct(a, rel)})
            elif isinstance(a, int) and not isinstance(a, bool):
                args.append(a if abs(a) < 2 ** 32 else "addr")  # (a bare address argument: device pointers lie above)
            else:
                args.append(a)
        steps.append({"fn": name, "what": st.what, "args": args})
    return steps


def pack(steps: list, names: list) -> dict:
    """A plan's steps in the short form: their numbers in `names` (extended as needed), one digest over all records,
    and the records of the session's own launches by step index."""
    idx = []
    for st in steps:
        key = f"{st['fn']} {st['what']}"
        if key not in names:
            names.append(key)
        idx.append(names.index(key))
    text = json.dumps([st["args"] for st in steps], sort_keys=True)
    return {"steps": idx, "sha1": hashlib.sha1(text.encode()).hexdigest(),
            "tail": {str(i): st["args"] for i, st in enumerate(steps) if st["fn"] in TAIL}}


def session_fingerprint(s, names=None) -> dict:
    """names: the shared table, for the short form; None: every record in full."""
    plans = [plan_fingerprint(p, s, c) for p, c in zip(s.plans, s.children or [s])]
    return {"children": [c.batch for c in s.children],
            "plans": plans if names is None else [pack(p, names) for p in plans]}


def dump(device="meta", split=False, fp8=None, full=False, which="dbl") -> dict:
    """which: "dbl" (VARIANTS), "heads" (HEADS) or "all"."""
    rows = []
    if which != "heads":
        rows += [(name, "yolov13n_DBL.yaml", cls, kw) for name, cls, kw in VARIANTS]
    if which != "dbl":
        rows += [(name, str(ROOT / "tests" / "golden" / cfg), cls, kw) for name, cfg, cls, kw in HEADS]
    names = None if full else []
    out, models = {}, {}
    for name, cfg, cls, kw in rows:
        if cfg not in models:
            torch.manual_seed(0)
            models[cfg] = YOLO(cfg, nc=3).model
        model = models[cfg]
        out[name] = session_fingerprint(cls(model, 2, H, W, device=device, **kw), names)
        if split and name in SPLIT:
            out[name + "_split"] = session_fingerprint(cls(model, 5, H, W, device=device, streams=2, **kw), names)
    if fp8:
        torch.manual_seed(0)
        model = YOLO("yolov13s_DBL.yaml", nc=3).model
        s = DetectSession(model, 2, H, W, dtype=torch.float16, device=device, fp8=0.1, fp8_calibration=str(fp8))
        s.calibrate_fp8(calibration=s.fp8_calibration)
        out["detect_fp8"] = session_fingerprint(s, names)
    return {"sessions": out} if full else {"names": names, "sessions": out}


def format_dump(d: dict) -> str:
    """One line for the table, one per session."""
    rows = [f'{json.dumps(k)}: {json.dumps(v, sort_keys=True, separators=(",", ":"))}'
            for k, v in sorted(d["sessions"].items())]
    head = f'"names": {json.dumps(d["names"], separators=(",", ":"))},\n' if "names" in d else ""
    return "{\n" + head + '"sessions": {\n' + ",\n".join(rows) + "\n}\n}\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--device", default="meta")
    ap.add_argument("--split", action="store_true", help="add the batch 5, streams=2 forms")
    ap.add_argument("--fp8", default=None, help="an Fp8Calibration file: add one DBL-s fp8=0.1 session")
    ap.add_argument("--full", action="store_true", help="every step's descriptors in full, not only the tail's")
    ap.add_argument("--list", default="dbl", choices=("dbl", "heads", "all"), dest="which",
                    help="the YOLOv13-DBL matrix, the end2end / Segment heads, or both")
    ap.add_argument("--out", default=None, help="write here instead of stdout")
    a = ap.parse_args()
    text = format_dump(dump(a.device, a.split, a.fp8, a.full, a.which))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
