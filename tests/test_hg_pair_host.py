"""HyperACE's paired AdaHGConv launch without a GPU: the launch order around the pair on the meta device (DBL-n and
DBL-s), the YDBL_NO_HG_PAIR switch restoring the parent's list of launches, the switch being part of the plan-cache
key, and the C-ABI export with its null-descriptor check."""

from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


def _whats(cfg, dtype=torch.float16):
    from ydbl import YOLO

    torch.manual_seed(0)
    cm = YOLO(cfg, nc=3).model.compile(2, 96, 128, dtype, device="meta")
    return [st.what for st in cm.plan.steps], [st.fn.__name__ for st in cm.plan.steps]


@pytest.mark.parametrize("cfg", ["yolov13n_DBL.yaml", "yolov13s_DBL.yaml"])
def test_launch_order_and_switch(cfg, monkeypatch):
    monkeypatch.delenv("YDBL_NO_HG_PAIR", raising=False)
    whats, fns = _whats(cfg)
    assert whats.count("AdaHG.fused2") == 1 and "AdaHG.fused" not in whats
    k = whats.index("AdaHG.fused2")
    assert fns[k] == "ydbl_hg_fused_pair"
    # merged input 1x1s -> pair -> b2.cv3 -> b1.cv3
    assert whats[k - 1] == "C3AHx2.cv1|cv2"
    assert whats[k + 1 : k + 3] == ["Conv1x1", "Conv1x1"] and fns[k + 1 : k + 3] == ["ydbl_conv2d_nhwc"] * 2
    monkeypatch.setenv("YDBL_NO_HG_PAIR", "1")
    whats0, fns0 = _whats(cfg)
    # the parent's list: AdaHG.fused, b2.cv3, AdaHG.fused, b1.cv3 in place of the pair and the two cv3
    assert "AdaHG.fused2" not in whats0 and "ydbl_hg_fused_pair" not in fns0
    assert whats0[k - 1 : k + 4] == ["C3AHx2.cv1|cv2", "AdaHG.fused", "Conv1x1", "AdaHG.fused", "Conv1x1"]
    assert fns0[k : k + 4] == ["ydbl_hg_fused", "ydbl_conv2d_nhwc", "ydbl_hg_fused", "ydbl_conv2d_nhwc"]
    assert len(whats0) == len(whats) + 1
    assert whats0[:k] == whats[:k] and whats0[k + 4 :] == whats[k + 3 :]


def test_pair_descriptors_are_the_branch_slices(monkeypatch):
    """d0 = branch2 (bb[2c_:3c_] -> bb[0:c_]), d1 = branch1 (bb[3c_:4c_] -> bb[5c_:6c_]): one buffer, disjoint
    channel ranges, two workspaces."""
    from ydbl import YOLO

    monkeypatch.delenv("YDBL_NO_HG_PAIR", raising=False)
    cm = YOLO("yolov13n_DBL.yaml", nc=3).model.compile(2, 96, 128, torch.float16, device="meta")
    (st,) = [st for st in cm.plan.steps if st.what == "AdaHG.fused2"]
    d0, d1 = st.args
    c_ = d0.x.c
    assert d0.x.cs == d1.x.cs == d0.y.cs == d1.y.cs == 6 * c_ and d1.x.c == d0.y.c == d1.y.c == c_
    assert (d0.x.n, d0.x.h, d0.x.w) == (d1.x.n, d1.x.h, d1.x.w) == (2, 6, 8)
    assert d0.num_edges == d1.num_edges and d0.num_heads == d1.num_heads == c_ // 16


def test_staged_route_never_pairs(monkeypatch):
    monkeypatch.delenv("YDBL_NO_HG_PAIR", raising=False)
    monkeypatch.setenv("YDBL_HG_UNFUSED", "1")
    whats, fns = _whats("yolov13n_DBL.yaml")
    assert "ydbl_hg_fused_pair" not in fns and "ydbl_hg_fused" not in fns and whats.count("AdaHG.propagate") == 2


def test_switch_is_part_of_the_plan_cache_key(monkeypatch):
    from ydbl.runtime import SWITCHES, ydbl_env

    assert "YDBL_NO_HG_PAIR" in SWITCHES
    monkeypatch.delenv("YDBL_NO_HG_PAIR", raising=False)
    a = ydbl_env()
    monkeypatch.setenv("YDBL_NO_HG_PAIR", "1")
    assert ydbl_env() != a


def test_export_signature_and_null_descriptors():
    from ydbl import _lib

    assert "ydbl_hg_fused_pair" in _lib.SIGNATURES and hasattr(_lib.lib, "ydbl_hg_fused_pair")
    assert "ydbl_hg_fused_pair" in (ROOT / "include" / "ydbl.h").read_text()
    d = _lib.HgDesc()
    assert _lib.lib.ydbl_hg_fused_pair(None, None, None) == 1
    assert "null descriptor" in _lib.lib.ydbl_last_error().decode()
    assert _lib.lib.ydbl_hg_fused_pair(d, None, None) == 1 and _lib.lib.ydbl_hg_fused_pair(None, d, None) == 1
    # two empty descriptors fail ydbl_hg_fused's own checks: the fallback returns the first call's error, no launch
    assert _lib.lib.ydbl_hg_fused_pair(d, d, None) == 1
