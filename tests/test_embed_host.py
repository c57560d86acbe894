"""embed() without a GPU: index normalisation, the rejected combinations (raised before any device is touched), the
truncated launch plan on the meta device, and the C-ABI of ydbl_global_avgpool (exports, descriptor layout against
gcc, argument validation)."""

import ctypes as C
import subprocess
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ydbl.h"


@pytest.fixture(scope="module")
def yolo():
    from ydbl import YOLO

    return YOLO("yolov13n_DBL.yaml", nc=3)


# ---------------------------------------------------------------------------------------------- indices
def test_normalize_sorts_and_dedups(yolo):
    from ydbl.nn.tasks import normalize_embed

    n = len(yolo.model.model)
    assert n == 36
    assert normalize_embed([34, 1, 34, 9], n) == (1, 9, 34)
    assert normalize_embed((0,), n) == (0,)
    assert normalize_embed([torch.tensor(3)], n) == (3,)


@pytest.mark.parametrize("bad", [[-1], [35], [36], [1.5], [True], ["9"], [9, 40]])
def test_normalize_rejects(yolo, bad):
    from ydbl.nn.tasks import normalize_embed

    with pytest.raises(ValueError, match=r"0\.\.34"):
        normalize_embed(bad, len(yolo.model.model))


@pytest.mark.parametrize("given", [None, []])
def test_embed_defaults_to_second_to_last_layer(yolo, given, monkeypatch):
    seen = {}
    monkeypatch.setattr(type(yolo), "predict", lambda self, source=None, stream=False, **kw: seen.update(kw) or "ret")
    kw = {} if given is None else {"embed": given}
    assert yolo.embed("src", **kw) == "ret"
    assert seen["embed"] == [len(yolo.model.model) - 2] == [34]
    yolo.embed("src", embed=[3, 1])
    assert seen["embed"] == [3, 1]


def test_defaults_carry_embed():
    from ydbl.engine.model import DEFAULTS

    assert "embed" in DEFAULTS and DEFAULTS["embed"] is None


# ---------------------------------------------------------------------------------------------- rejected combinations
@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to pick a device fails the test: the guards must fire first."""
    import ydbl.engine.model as em

    def boom(*a, **k):
        raise AssertionError("a device was selected before the embed guards ran")

    monkeypatch.setattr(em, "select_device", boom)


def test_rejected_before_any_device(yolo, no_device):
    x = torch.zeros(2, 3, 96, 128)
    with pytest.raises(ValueError, match="augment"):
        yolo.predict(x, embed=[34], augment=True)
    with pytest.raises(ValueError, match="augment"):
        yolo.session(2, 96, 128, embed=[34], augment=True)
    with pytest.raises(ValueError, match="augment"):
        yolo.model(x, embed=[34], augment=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        yolo.predict(x, embed=[34], fp8=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        yolo.session(2, 96, 128, embed=[34], fp8=True)
    with pytest.raises(NotImplementedError, match="gather_rows"):
        yolo.session(2, 96, 128, embed=[34], gather_rows=4)
    for bad in ([-1], [35], [36], [1.5]):
        with pytest.raises(ValueError, match=r"0\.\.34"):
            yolo.predict(x, embed=bad)
        with pytest.raises(ValueError, match=r"0\.\.34"):
            yolo.embed(x, embed=bad)
        with pytest.raises(ValueError, match=r"0\.\.34"):
            yolo.session(2, 96, 128, embed=bad)
        with pytest.raises(ValueError, match=r"0\.\.34"):
            yolo.model(x, embed=bad)


def test_forward_still_rejects_profile_and_visualize(yolo):
    x = torch.zeros(1, 3, 64, 64)
    for k in ("profile", "visualize"):
        with pytest.raises(NotImplementedError, match="profile / visualize are"):
            yolo.model(x, **{k: True})


# ---------------------------------------------------------------------------------------------- the plan (meta device)
def test_truncated_plan_on_meta(yolo):
    full = yolo.model.compile(2, 96, 128, torch.float16, device="meta")
    cm = yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(9, 34))
    whats = [st.what for st in cm.plan.steps]
    assert not any(w.startswith("Detect") for w in whats)
    assert whats.count("embed.pool") == 2 and whats[-1] == "embed.pool"
    assert cm.embed_out.shape == (2, 128 + 256) and cm.embed_out.dtype == torch.float16
    assert cm.levels is None and cm.embed == (9, 34)
    assert full.levels is not None and full.embed_out is None
    assert len(cm.plan.steps) < len(full.plan.steps)
    short = yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(9,))
    assert len(short.plan.steps) < len(cm.plan.steps)
    assert short.plan.bytes_allocated < cm.plan.bytes_allocated < full.plan.bytes_allocated
    cm.plan.check_single_stream()
    # the order of the list and repeats change nothing
    again = yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=[34, 9, 34])
    assert [st.what for st in again.plan.steps] == whats


def test_pool_sits_right_behind_its_layer(yolo):
    """The pool of layer i is emitted before the first launch of layer i + 1: the plan of embed=(9, 34) up to its
    first pool is exactly the plan of embed=(9,)."""
    a = [st.what for st in yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(9,)).plan.steps]
    b = [st.what for st in yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(9, 34)).plan.steps]
    assert b[: len(a)] == a


def test_pool_descriptors(yolo):
    cm = yolo.model.compile(2, 96, 128, torch.float32, device="meta", embed=(1, 9, 34))
    pools = [st.args[0] for st in cm.plan.steps if st.what == "embed.pool"]
    assert [d.x.c for d in pools] == [16, 128, 256] and cm.embed_out.shape == (2, 400)
    assert all(d.y_stride == 400 and d.x.n == 2 for d in pools)
    assert [(d.x.h, d.x.w) for d in pools] == [(48, 64), (6, 8), (3, 4)]  # strides 2, 16, 32
    assert set(cm.embed_views) == {1, 9, 34}


def test_embed_layer0_drops_the_stem2_fusion(yolo):
    full = yolo.model.compile(2, 96, 128, torch.float16, device="meta")
    assert any(st.fn.__name__ == "ydbl_conv_stem2" for st in full.plan.steps)  # the fusion this plan must not take
    cm = yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(0,))
    assert not any(st.fn.__name__ == "ydbl_conv_stem2" for st in cm.plan.steps)
    pools = [st.args[0] for st in cm.plan.steps if st.what == "embed.pool"]
    assert len(pools) == 1 and (pools[0].x.h, pools[0].x.w) == (96, 128)
    both = yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(0, 1))
    assert not any(st.fn.__name__ == "ydbl_conv_stem2" for st in both.plan.steps)
    one = yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(1,))
    assert any(st.fn.__name__ == "ydbl_conv_stem2" for st in one.plan.steps)  # layer 1 alone keeps it


def test_caller_supplied_output_rows(yolo):
    out = torch.empty((5, 256), dtype=torch.float16, device="meta")
    cm = yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(34,), embed_out=out[3:5])
    assert cm.embed_out.shape == (2, 256)
    with pytest.raises(ValueError, match="embed_out"):
        yolo.model.compile(2, 96, 128, torch.float16, device="meta", embed=(34,), embed_out=out)


# ---------------------------------------------------------------------------------------------- C-ABI
def test_exports_and_signatures():
    from ydbl import _lib

    for name in ("ydbl_global_avgpool", "ydbl_global_avgpool_workspace"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES
        assert name in HEADER.read_text()


def test_desc_layout_matches_c(tmp_path):
    from ydbl import _lib

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ydbl_avgpool_desc));']
    for fname, _ in _lib.AvgPoolDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(ydbl_avgpool_desc, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split() for line in out if line.strip())
    assert int(got["size"]) == C.sizeof(_lib.AvgPoolDesc)
    for fname, _ in _lib.AvgPoolDesc._fields_:
        assert int(got[fname]) == getattr(_lib.AvgPoolDesc, fname).offset, fname


def _desc(ptr=4096, n=2, h=80, w=80, c=16, cs=16, dtype=1, y=8192, y_stride=16, ws=None, ws_bytes=0):
    from ydbl import _lib

    return _lib.AvgPoolDesc(_lib.View(ptr, n, h, w, c, cs, dtype), y, y_stride, ws, ws_bytes)


def test_validation_errors_launch_nothing():
    """Every rejected descriptor returns YDBL_EINVAL (1) with a message, from the argument checks ahead of any launch
    (the pointers are made up: a launch would not return an error code here, there is no device)."""
    from ydbl import _lib

    lib = _lib.lib
    err = lambda: lib.ydbl_last_error().decode()  # noqa: E731
    assert lib.ydbl_global_avgpool(None, None) == 1 and "null descriptor" in err()
    assert lib.ydbl_global_avgpool(_desc(ptr=None), None) == 1 and "null pointer" in err()
    assert lib.ydbl_global_avgpool(_desc(y=None), None) == 1 and "null pointer" in err()
    assert lib.ydbl_global_avgpool(_desc(dtype=7), None) == 1 and "dtype" in err()
    assert lib.ydbl_global_avgpool(_desc(h=0), None) == 1 and "empty view" in err()
    assert lib.ydbl_global_avgpool(_desc(c=16, cs=8), None) == 1 and "shape" in err()
    assert lib.ydbl_global_avgpool(_desc(y_stride=15), None) == 1 and "y_stride" in err()
    need = lib.ydbl_global_avgpool_workspace(_desc())
    assert need > 0
    assert lib.ydbl_global_avgpool(_desc(), None) == 1 and "workspace" in err()
    assert lib.ydbl_global_avgpool(_desc(ws=1 << 20, ws_bytes=need - 1), None) == 1 and "workspace" in err()
    assert lib.ydbl_global_avgpool_workspace(_desc(dtype=7)) == -1


def test_workspace_depends_on_the_map_not_the_batch():
    """chunks = f(h*w, c, dtype): the bytes scale linearly with n, and a map of one chunk needs none."""
    from ydbl import _lib

    ws = _lib.lib.ydbl_global_avgpool_workspace
    for dtype in (0, 1):
        one = ws(_desc(n=1, dtype=dtype))
        assert one > 0 and one % (16 * 4) == 0
        assert ws(_desc(n=5, dtype=dtype)) == 5 * one
        assert ws(_desc(n=3, h=3, w=4, c=256, cs=256, dtype=dtype)) == 0
    assert ws(_desc(n=1, h=1, w=1, c=8, cs=8)) == 0
