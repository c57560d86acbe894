"""The YOLOv13 baseline (yolov13.yaml: A2C2f, grouped Conv, nn.Upsample) on the host: construction for n/s/l/x
from tests/golden/yolov13.json, reference parameter names and shapes, the YAML route with 'None' as a string, the
scope guards, the descriptor layout -- and the yardstick (tests/a2c2f_util.py) checked against torch's own
scaled_dot_product_attention.  No GPU."""

import ctypes as C
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import a2c2f_util as U

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("scale", ["n", "s", "l", "x"])
def test_constructs_with_reference_names_and_shapes(scale, golden_dir):
    from ydbl import YOLO

    p = YOLO(str(golden_dir / f"yolov13{scale}.json"), nc=3)
    o = U.build_oracle(scale, 3)
    sp, so = p.model.state_dict(), o.state_dict()
    assert list(sp) == list(so)
    assert all(sp[k].shape == so[k].shape for k in so)
    assert p.model.stride.tolist() == [8.0, 16.0, 32.0]
    assert p.model.model[-1].legacy is False
    gammas = [k for k in sp if k.endswith(".gamma")]
    assert bool(gammas) == (scale in "lx")  # the residual form (True, 1.5) is the l / x scale rule
    if scale == "n":
        assert sum(t.numel() for t in p.model.parameters()) == 2_478_928
        assert sum(t.numel() for t in o.parameters()) == 2_478_928
    p.model.load_state_dict(so, strict=True)


def test_yaml_with_none_string_parses_like_the_json(tmp_path, golden_dir):
    """yolov13n.yaml resolves to a yolov13.yaml beside it at scale n; YAML delivers [None, 2, "nearest"] with 'None'
    as a string."""
    import json

    import yaml

    from ydbl import YOLO
    from ydbl.nn.tasks import yaml_model_load

    d = json.loads((golden_dir / "yolov13.json").read_text())
    text = yaml.safe_dump(d, default_flow_style=None).replace("null", "None")
    (tmp_path / "yolov13.yaml").write_text(text)
    loaded = yaml_model_load(tmp_path / "yolov13n.yaml")
    assert loaded["scale"] == "n"
    ups = [layer for layer in loaded["head"] if layer[2] == "nn.Upsample"]
    assert len(ups) == 3 and all(layer[3] == ["None", 2, "nearest"] for layer in ups)
    a = YOLO(str(tmp_path / "yolov13n.yaml"), nc=3)
    b = YOLO(str(golden_dir / "yolov13n.json"), nc=3)
    assert [(k, tuple(v.shape)) for k, v in a.model.state_dict().items()] == [
        (k, tuple(v.shape)) for k, v in b.model.state_dict().items()]
    up = a.model.model[10]
    assert up.size is None and up.scale_factor == 2 and up.mode == "nearest"
    assert a.model.model[9].branch1.m.hgnn.edge_generator.context == "both"  # strings that are no literals stay


def test_scope_guards():
    from ydbl.nn.modules import A2C2f, Upsample

    with pytest.raises(NotImplementedError):
        A2C2f(64, 64, 1, False, 1)
    for args in ((None, 4, "nearest"), (None, 2, "bilinear"), ((8, 8), None, "nearest")):
        with pytest.raises(NotImplementedError):
            Upsample(*args)
    x = torch.rand(1, 3, 4, 5)
    assert torch.equal(Upsample(None, 2, "nearest")(x), F.interpolate(x, scale_factor=2.0, mode="nearest"))


def test_fp8_on_a_model_with_a2c2f_raises(golden_dir):
    from ydbl import YOLO
    from ydbl.engine.session import DetectSession

    p = YOLO(str(golden_dir / "yolov13n.json"), nc=3)
    with pytest.raises(NotImplementedError, match="A2C2f"):  # raised before any device work
        DetectSession(p.model, 1, 64, 64, torch.float16, fp8=True)


def test_area_attn_desc_layout_matches_c(tmp_path):
    from ydbl import _lib

    header = ROOT / "include" / "ydbl.h"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ydbl_area_attn_desc));']
    for name, _ in _lib.AreaAttnDesc._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof(ydbl_area_attn_desc, {name}));')
    lines.append("return 0;}")
    (tmp_path / "l.c").write_text("\n".join(lines))
    subprocess.run(["gcc", str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.AreaAttnDesc)
    for name, _ in _lib.AreaAttnDesc._fields_:
        assert int(got[name]) == getattr(_lib.AreaAttnDesc, name).offset
    assert _lib.lib.ydbl_area_attn(None, None) == 1
    assert _lib.lib.ydbl_channel_gate_add(None, None, None, None, None) == 1


@pytest.mark.parametrize("n,h,w,heads,area", [(2, 6, 10, 2, 4), (1, 20, 20, 4, 1), (2, 4, 4, 1, 1), (1, 8, 8, 2, 4)])
def test_restatement_core_equals_sdpa(n, h, w, heads, area):
    """The yardstick guards itself: in fp64 its AAttn core equals F.scaled_dot_product_attention on the same
    per-chunk q / k / v to 1e-12 (area 1 and 4, T = 15 included)."""
    g = torch.Generator().manual_seed(n * 1000 + h * w + area)
    C_ = heads * 32
    qkv = torch.randn(n, 3 * C_, h, w, generator=g, dtype=torch.float64)
    a = U.AAttn(C_, heads, area)
    y, v = a.core(qkv)
    q, k, vv = a.split(qkv, n, C_, h * w)  # [B*area, heads, 32, T]
    T = h * w // area
    assert q.shape == (n * area, heads, 32, T)
    ref = F.scaled_dot_product_attention(q.transpose(-2, -1), k.transpose(-2, -1), vv.transpose(-2, -1))  # [Ba,hd,T,32]
    ref = ref.permute(0, 2, 1, 3).reshape(n, h * w, C_).reshape(n, h, w, C_).permute(0, 3, 1, 2)
    assert (y - ref).abs().max().item() <= 1e-12
    vref = vv.permute(0, 3, 1, 2).reshape(n, h, w, C_).permute(0, 3, 1, 2)
    assert torch.equal(v, vref)
    # v is the V channels of qkv, token for token
    tok = qkv.permute(0, 2, 3, 1).reshape(n, h, w, heads, 96)[..., 64:].reshape(n, h, w, C_).permute(0, 3, 1, 2)
    assert torch.equal(v, tok)
