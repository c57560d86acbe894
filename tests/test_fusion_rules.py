"""Host-side fusion rules of the plan builder (no GPU)."""
from ydbl.nn import modules as M


def test_dwpw_fused_default_at_64_outputs(monkeypatch):
    """The Detect DWConv -> Conv1x1 pairs run as one launch at 64 pointwise outputs (DBL-n) and as two at 128+
    (DBL-s / DBL-l), unless YDBL_DWPW forces either (profiles/r06/r06_detect_switch_sweep.txt)."""
    monkeypatch.delenv("YDBL_DWPW", raising=False)
    assert M.dwpw_fuse(64) and not M.dwpw_fuse(128)
    monkeypatch.setenv("YDBL_DWPW", "1")
    assert M.dwpw_fuse(128)
    monkeypatch.setenv("YDBL_DWPW", "0")
    assert not M.dwpw_fuse(64)

