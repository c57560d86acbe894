"""The session classes without a GPU, on the meta device: the launch plans of a fixed matrix of sessions against the
fingerprint recorded before the classes were unified (tests/golden/session_plans_meta.json, written by
scripts/session_plan_dump.py), the split layout by property, the options record as the session-cache key, and the
calls an augmented session does not support."""

import dataclasses
import importlib.util
import json
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def dump():
    spec = importlib.util.spec_from_file_location("session_plan_dump", ROOT / "scripts" / "session_plan_dump.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def model():
    from ydbl import YOLO

    torch.manual_seed(0)
    return YOLO("yolov13n_DBL.yaml", nc=3).model


def test_plans_equal_the_recorded_fingerprint(dump):
    want = json.loads((ROOT / "tests" / "golden" / "session_plans_meta.json").read_text())
    got = json.loads(dump.format_dump(dump.dump("meta")))
    assert sorted(got["sessions"]) == sorted(want["sessions"]) == sorted(name for name, _, _ in dump.VARIANTS)
    assert got["names"] == want["names"]
    for name, fp in want["sessions"].items():  # (scripts/session_plan_dump.py --full shows where a digest differs)
        assert got["sessions"][name] == fp, name


def test_head_plans_equal_the_recorded_fingerprint(dump):
    """The end2end (decode_e2e + top-k) and Segment (NMS with keep_idx) tails, as recorded before the tail moved into
    ydbl/tail.py (tests/golden/session_plans_heads_meta.json: scripts/session_plan_dump.py --list heads)."""
    want = json.loads((ROOT / "tests" / "golden" / "session_plans_heads_meta.json").read_text())
    got = json.loads(dump.format_dump(dump.dump("meta", which="heads")))
    assert sorted(got["sessions"]) == sorted(want["sessions"]) == sorted(name for name, *_ in dump.HEADS)
    assert got["names"] == want["names"]
    for name, fp in want["sessions"].items():
        assert got["sessions"][name] == fp, name


def _rows(t, parent):
    """(first row, rows) of `t`, a slice of `parent` along dim 0 (meta tensors have no address: storage offsets)."""
    assert t.stride() == parent.stride() and t.shape[1:] == parent.shape[1:]
    off = t.storage_offset() - parent.storage_offset()
    assert off % parent.stride(0) == 0
    return off // parent.stride(0), t.shape[0]


@pytest.mark.parametrize("name", ["detect_fp16", "detect_fp16_val", "detect_pred_no_nms", "augment", "augment_pred",
                                  "embed"])
def test_split_session_on_meta(dump, model, name):
    """Batch 5 on two streams builds on the meta device (no stream exists before an eager split launch), splits as
    [(0, 3), (3, 5)], and each child is the unsplit session of its batch, built onto its rows of the shared outputs."""
    cls, kw = next((c, k) for n, c, k in dump.VARIANTS if n == name)
    s = cls(model, 5, dump.H, dump.W, device="meta", streams=2, **kw)
    assert s.bounds == [(0, 3), (3, 5)] and [c.batch for c in s.children] == [3, 2]
    assert s.plans == [c.plan for c in s.children] and s.plan is s.plans[0]
    for c, (a, b) in zip(s.children, s.bounds):
        alone = cls(model, b - a, dump.H, dump.W, device="meta", **kw)
        assert alone.children == [] and alone.bounds == [(0, b - a)] and alone.plans == [alone.plan]
        # relative to its own slices the child's plan is the unsplit session's, descriptor for descriptor ...
        assert dump.plan_fingerprint(c.plan, c, c) == dump.plan_fingerprint(alone.plan, alone, alone)
        for st in dump.plan_fingerprint(c.plan, s, c):  # ... and relative to the shared outputs it writes its rows
            if st["fn"] == "ydbl_nms":
                nd = st["args"][0]["NmsDesc"]
                assert (nd["out"], nd["out_count"]) == ({"off": a * s.max_det * 6 * 4}, {"off": a * 4})
            elif st["fn"].startswith("ydbl_detect_decode") and kw.get("keep_pred"):
                assert st["args"][0]["DecodeDesc"]["y_ref"] == {"off": a * s.pred.stride(0) * 4}
        outs = [("out",)] if name == "embed" else [("det",), ("count",)] + ([("pred",)] if kw.get("keep_pred") else [])
        for (attr,) in outs:
            assert _rows(getattr(c, attr), getattr(s, attr)) == (a, b - a), attr
    if name != "embed":
        assert s.cand_count.shape == (5,) and (s.pred is None) == (not kw.get("keep_pred"))


def _key(opt, **kw):
    from ydbl.engine.model import session_key

    place = dict(batch=2, h=96, w=128, dev=torch.device("cuda", 0), streams=1, gather_rows=None, augment=False)
    return session_key(opt, **{**place, **kw})


OTHER = {"dtype": torch.float32, "conf": 0.3, "iou": 0.5, "max_det": 100, "multi_label": True, "agnostic": True,
         "classes": (0, 2), "max_nms": 1000, "max_wh": 4096.0, "clip": False, "keep_pred": True, "use_graph": False,
         "nms": False, "fp8": 0.25, "fp8_calibration": "calibration.json", "loss": {"max_labels": 8}}


def test_every_option_is_in_the_session_key():
    from ydbl.engine.session import DetectOptions

    names = [f.name for f in dataclasses.fields(DetectOptions)]
    assert sorted(names) == sorted(OTHER), "a new option needs a second value here"
    base = DetectOptions()
    assert _key(base) == _key(DetectOptions()) and hash(_key(base)) == hash(_key(DetectOptions()))
    keys = {_key(base)}
    for name in names:
        changed = dataclasses.replace(base, **{name: OTHER[name]})
        assert _key(changed) != _key(base), name
        assert _key(changed) == _key(dataclasses.replace(base, **{name: OTHER[name]})), name
        keys.add(_key(changed))
    assert len(keys) == len(names) + 1
    assert _key(DetectOptions(classes=[0, 2])) == _key(DetectOptions(classes=(0, 2)))
    assert DetectOptions(classes=[0, 2]).classes == (0, 2)
    for place in (dict(batch=3), dict(h=64), dict(w=64), dict(dev=torch.device("cuda", 1)), dict(streams=2),
                  dict(gather_rows=2), dict(augment=True)):
        assert _key(base, **place) != _key(base), place
    with pytest.raises(dataclasses.FrozenInstanceError):
        base.conf = 0.5


def test_constructors_take_the_record_or_the_settings(model):
    from ydbl.engine.session import DetectOptions, DetectSession

    a = DetectSession(model, 2, 96, 128, torch.float16, 0.3, 0.5, classes=[0, 2], device="meta")
    assert a.opt == DetectOptions(torch.float16, 0.3, 0.5, classes=(0, 2))
    b = DetectSession(model, 2, 96, 128, device="meta", options=a.opt)
    assert b.opt is a.opt and (b.conf, b.iou, b.max_det) == (0.3, 0.5, 300)
    with pytest.raises(TypeError):
        DetectSession(model, 2, 96, 128, conf=0.3, device="meta", options=a.opt)
    with pytest.raises(TypeError):
        DetectSession(model, 2, 96, 128, device="meta", no_such_option=1)
    s = DetectSession(model, 5, 96, 128, device="meta", streams=2, options=a.opt)
    assert all(c.opt is a.opt for c in s.children)  # the record itself, not a re-spelled argument list


@pytest.mark.parametrize("streams", [1, 2])
def test_augment_states_what_it_does_not_support(model, streams):
    from ydbl.engine.session import AugmentSession

    s = AugmentSession(model, 4, 96, 128, torch.float16, device="meta", streams=streams)
    x = torch.zeros((4, 3, 96, 128), dtype=torch.float32, device="meta")
    assert s.can_bind(x) is False
    with pytest.raises(ValueError, match="launch_bound"):
        s.launch_bound(x)
    with pytest.raises(RuntimeError, match="without loss="):
        s.load_labels(torch.zeros((4, 8, 5)))
    with pytest.raises(NotImplementedError, match="fp8"):
        s.calibrate_fp8()
    assert s.loss is None and s.records is None and s.fp8 is False and s.feats() is None
    with pytest.raises(NotImplementedError, match="fp8"):
        AugmentSession(model, 2, 96, 128, torch.float16, device="meta", fp8=True)
    with pytest.raises(ValueError, match="loss"):
        AugmentSession(model, 2, 96, 128, torch.float16, device="meta", loss={"max_labels": 8})
