"""The YOLO11 / YOLOv8 baselines (yolo11.yaml: C3k2, SPPF, C2PSA; yolov8.yaml: C2f, SPPF) on the host: construction at
n and s from tests/golden/yolo11.json / yolov8.json, reference parameter names and shapes, the legacy flag, the parser
rules, the YAML route, the two new descriptors' layouts, the refusals of the two new entry points, the fp8 guard --
and the yardstick (tests/yolo11_util.py) checked against torch's own scaled_dot_product_attention and against a
direct windowed maximum.  No GPU."""

import ctypes as C
import json
import subprocess
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import yolo11_util as U

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("scale", ["n", "s"])
@pytest.mark.parametrize("family", ["yolo11", "yolov8"])
def test_constructs_with_reference_names_and_shapes(family, scale, golden_dir):
    from ydbl import YOLO
    from ydbl.nn import modules as M

    p = YOLO(str(golden_dir / f"{family}{scale}.json"), nc=3)
    o = U.build_oracle(family, scale, 3)
    sp, so = p.model.state_dict(), o.state_dict()
    assert list(sp) == list(so)
    assert all(sp[k].shape == so[k].shape for k in so)
    assert p.model.stride.tolist() == [8.0, 16.0, 32.0]
    head = p.model.model[-1]
    if family == "yolo11":
        assert head.legacy is False
        assert all(isinstance(seq[0][0], M.DWConv) and isinstance(seq[1][0], M.DWConv) for seq in head.cv3)
        psa = p.model.model[10]
        assert isinstance(psa, M.C2PSA) and len(psa.m) == 1  # 2 repeats x depth 0.5
        assert (psa.m[0].attn.head_dim, psa.m[0].attn.key_dim) == (64, 32)
        assert psa.m[0].attn.num_heads == {"n": 2, "s": 4}[scale]
    else:
        assert head.legacy is True
        assert all(isinstance(seq[0], M.Conv) and seq[0].conv.kernel_size == (3, 3) for seq in head.cv3)
    assert isinstance(p.model.model[9], M.SPPF)
    p.model.load_state_dict(so, strict=True)


def test_legacy_flag_survives_a_second_model(golden_dir):
    """Detect.legacy is set on the class, as the reference does, and on the instance: building a yolov8 model after a
    yolo11 one must not flip the first head into the branch its cv3 was not built for (and back)."""
    from ydbl import YOLO

    a = YOLO(str(golden_dir / "yolo11n.json"), nc=3)
    b = YOLO(str(golden_dir / "yolov8n.json"), nc=3)
    c = YOLO(str(golden_dir / "yolo11n.json"), nc=3)
    assert (a.model.model[-1].legacy, b.model.model[-1].legacy, c.model.model[-1].legacy) == (False, True, False)
    for m in (a, b, c):  # every head still compiles (shape-only plan)
        assert len(m.model.compile(1, 64, 64, torch.float16, device="meta").levels) == 3


def test_parser_rules_for_c3k2_and_c2psa():
    """[256, False, 0.25] -> C3k2(c1, 64, n, False, 0.25) with plain Bottlenecks at the default e=0.5; [1024, True] ->
    C3k blocks; the repeat count is an argument (U/nn/tasks.py:1057-1083), never an nn.Sequential of repeats; the
    commented-out scale rule (:1086-1087) is not applied at any scale."""
    from ydbl.nn import modules as M
    from ydbl.nn.tasks import parse_model

    d = {"nc": 3, "scales": {"n": [0.5, 0.25, 1024], "l": [1.0, 1.0, 512]}, "scale": "n",
         "backbone": [[-1, 1, "Conv", [64, 3, 2]], [-1, 2, "C3k2", [256, False, 0.25]], [-1, 2, "C3k2", [1024, True]],
                      [-1, 2, "C2PSA", [1024]]],
         "head": [[[1, 2, 3], 1, "Detect", ["nc"]]]}
    model, _ = parse_model(json.loads(json.dumps(d)))
    a, b, c = model[1], model[2], model[3]
    assert type(a) is M.C3k2 and len(a.m) == 1 and type(a.m[0]) is M.Bottleneck
    assert a.cv2.conv.out_channels == 64 and a.c == 16  # 256 * 0.25 wide, e = 0.25
    assert a.m[0].cv1.conv.out_channels == 8 and a.m[0].cv1.conv.kernel_size == (3, 3)  # Bottleneck's default e=0.5
    assert type(b) is M.C3k2 and len(b.m) == 1 and type(b.m[0]) is M.C3k and len(b.m[0].m) == 2
    assert b.m[0].m[0].cv1.conv.kernel_size == (3, 3) and b.m[0].m[0].cv1.conv.out_channels == 64  # e = 1.0 inside
    assert type(c) is M.C2PSA and len(c.m) == 1 and c.c == 128
    assert model[-1].legacy is False
    d["scale"] = "l"
    model, _ = parse_model(json.loads(json.dumps(d)))
    assert len(model[1].m) == 2 and all(type(m) is M.Bottleneck for m in model[1].m)  # no c3k=True rule for l / x
    assert type(model[3]) is M.C2PSA and len(model[3].m) == 2
    assert model[3].m[0].attn.num_heads == 4 and model[3].m[0].attn.head_dim == 64


def test_yaml_name_resolves_to_the_unified_file(tmp_path, golden_dir):
    import yaml

    from ydbl import YOLO
    from ydbl.nn.tasks import yaml_model_load

    d = json.loads((golden_dir / "yolo11.json").read_text())
    (tmp_path / "yolo11.yaml").write_text(yaml.safe_dump(d, default_flow_style=None).replace("null", "None"))
    loaded = yaml_model_load(tmp_path / "yolo11n.yaml")
    assert loaded["scale"] == "n" and loaded["backbone"][2][2] == "C3k2"
    a = YOLO(str(tmp_path / "yolo11n.yaml"), nc=3)
    b = YOLO(str(golden_dir / "yolo11n.json"), nc=3)
    assert [(k, tuple(v.shape)) for k, v in a.model.state_dict().items()] == [
        (k, tuple(v.shape)) for k, v in b.model.state_dict().items()]
    assert sum(t.numel() for t in a.model.parameters()) == sum(t.numel() for t in U.build_oracle("yolo11", "n", 3).parameters())


@pytest.mark.parametrize("family,name", [("yolo11", "C2PSA"), ("yolov8", "SPPF")])
def test_fp8_on_the_baselines_raises(family, name, golden_dir):
    from ydbl import YOLO
    from ydbl.engine.session import DetectSession

    p = YOLO(str(golden_dir / f"{family}n.json"), nc=3)
    with pytest.raises(NotImplementedError, match=name):  # raised before any device work
        DetectSession(p.model, 1, 64, 64, torch.float16, fp8=True)


def test_attention_with_other_dims_is_refused_at_emit():
    from ydbl.nn.modules import Attention
    from ydbl.runtime import Plan

    plan = Plan(torch.device("meta"), torch.float16)
    x = plan.alloc(1, 4, 4, 64)
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        Attention(64, 2, 0.5).emit(plan, x)


def _layout(tmp_path, cname, struct):
    header = ROOT / "include" / "ydbl.h"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void){",
             f'printf("size %zu\\n", sizeof({cname}));']
    for name, _ in struct._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof({cname}, {name}));')
    lines.append("return 0;}")
    (tmp_path / f"{cname}.c").write_text("\n".join(lines))
    subprocess.run(["gcc", str(tmp_path / f"{cname}.c"), "-o", str(tmp_path / cname)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / cname)], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(struct)
    for name, _ in struct._fields_:
        assert int(got[name]) == getattr(struct, name).offset


def test_new_desc_layouts_match_c(tmp_path):
    from ydbl import _lib

    _layout(tmp_path, "ydbl_psa_attn_desc", _lib.PsaAttnDesc)
    _layout(tmp_path, "ydbl_maxpool5_desc", _lib.MaxPool5Desc)


def _view(ptr, n, h, w, c, cs=None, dtype=1):
    from ydbl import _lib

    return _lib.View(ptr, n, h, w, c, cs or c, dtype)


def _refused(fn, d, word):
    """The call returns YDBL_EINVAL (1) before any launch and names the cause."""
    from ydbl import _lib

    assert fn(C.byref(d), None) == 1
    assert word in _lib.lib.ydbl_last_error().decode()


def test_entry_points_refuse_bad_descriptors():
    """Every descriptor here fails a check that precedes the launch: the made-up pointers are never dereferenced."""
    from ydbl import _lib

    pool, attn = _lib.lib.ydbl_maxpool5_cascade, _lib.lib.ydbl_psa_attn
    assert pool(None, None) == 1 and attn(None, None) == 1
    base = 0x10000
    xs = [_view(base + 32 * i, 1, 5, 7, 16, 64) for i in range(4)]  # four 16-channel slices of a 64-wide fp16 buffer
    _refused(pool, _lib.MaxPool5Desc(*xs, 3), "k must be 5")
    _refused(pool, _lib.MaxPool5Desc(*xs, 7), "k must be 5")
    _refused(pool, _lib.MaxPool5Desc(xs[0], _view(base + 34, 1, 5, 7, 16, 64), xs[2], xs[3], 5), "16-byte aligned")
    _refused(pool, _lib.MaxPool5Desc(xs[0], _view(base + 32, 1, 5, 7, 12, 64), xs[2], xs[3], 5), "16-byte aligned")
    _refused(pool, _lib.MaxPool5Desc(xs[0], _view(base + 16, 1, 5, 7, 16, 64), xs[2], xs[3], 5), "overlaps x")
    _refused(pool, _lib.MaxPool5Desc(xs[0], xs[1], xs[1], xs[3], 5), "outputs overlap")
    _refused(pool, _lib.MaxPool5Desc(xs[0], xs[1], xs[2], _view(base + 96, 1, 5, 6, 16, 64), 5), "shape")
    _refused(pool, _lib.MaxPool5Desc(xs[0], xs[1], xs[2], _view(base + 96, 1, 5, 7, 16, 64, 0), 5), "")

    qkv, y, v = _view(base, 2, 4, 4, 256), _view(base + 0x8000, 2, 4, 4, 128), _view(base + 0x10000, 2, 4, 4, 128)
    _refused(attn, _lib.PsaAttnDesc(qkv, y, v, 2, 32, 32, 0.1767767), "head_dim 64")
    _refused(attn, _lib.PsaAttnDesc(qkv, y, v, 2, 16, 64, 0.25), "key_dim 32")
    _refused(attn, _lib.PsaAttnDesc(qkv, y, v, 3, 32, 64, 0.1767767), "heads * 128")
    _refused(attn, _lib.PsaAttnDesc(qkv, _view(base + 0x8000, 2, 4, 4, 64), v, 2, 32, 64, 0.1767767), "heads*64")
    _refused(attn, _lib.PsaAttnDesc(qkv, _view(base + 0x8002, 2, 4, 4, 128), v, 2, 32, 64, 0.1767767),
             "16-byte aligned")
    _refused(attn, _lib.PsaAttnDesc(qkv, _view(base + 0x100, 2, 4, 4, 128), v, 2, 32, 64, 0.1767767), "overlap")
    _refused(attn, _lib.PsaAttnDesc(qkv, y, y, 2, 32, 64, 0.1767767), "overlap")
    big = _view(base, 70000, 1, 1, 256)
    _refused(attn, _lib.PsaAttnDesc(big, _view(base + (1 << 30), 70000, 1, 1, 128), _view(None, 0, 0, 0, 0, 0, 0), 2,
                                    32, 64, 0.1767767), "n <= 65535")


# ----------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("n,h,w,heads", [(2, 20, 20, 2), (1, 7, 9, 6), (2, 1, 1, 2)])
def test_restatement_core_equals_sdpa(n, h, w, heads):
    """The yardstick guards itself: in fp64 its Attention core equals F.scaled_dot_product_attention on the q / k / v
    cut out of the 128-channel head blocks by hand, to 1e-12."""
    g = torch.Generator().manual_seed(n * 1000 + h * w + heads)
    qkv = torch.randn(n, heads * 128, h, w, generator=g, dtype=torch.float64)
    a = U.Attention(heads * 64, heads, 0.5)
    assert (a.key_dim, a.head_dim) == (32, 64)
    y, v = a.core(qkv)
    blk = qkv.reshape(n, heads, 128, h * w)
    q, k, vv = blk[:, :, :32], blk[:, :, 32:64], blk[:, :, 64:]
    ref = F.scaled_dot_product_attention(q.transpose(-2, -1), k.transpose(-2, -1), vv.transpose(-2, -1))  # [n,hd,N,64]
    ref = ref.transpose(-2, -1).reshape(n, heads * 64, h, w)
    assert (y - ref).abs().max().item() <= 1e-12
    assert torch.equal(v, vv.reshape(n, heads * 64, h, w))
    yn, vn = U.psa_ref(qkv.permute(0, 2, 3, 1), heads, torch.float64)
    assert torch.equal(yn, y.permute(0, 2, 3, 1)) and torch.equal(vn, v.permute(0, 2, 3, 1))


def test_pool_cascade_equals_windowed_maxima():
    """What ydbl_maxpool5_cascade relies on: the chained 5x5 pools are the 5 / 9 / 13 windows, clipped (-inf padding)."""
    x = -torch.rand(1, 3, 5, 7, generator=torch.Generator().manual_seed(3)) - 0.5
    y = x
    for k in (5, 9, 13):
        y = F.max_pool2d(y, 5, 1, 2)
        assert torch.equal(y, F.max_pool2d(x, k, 1, k // 2))


MODULES = {
    "PSABlock": ("PSABlock", (128, 0.5, 2), 128),
    "C2PSA": ("C2PSA", (256, 256, 2), 256),
}


@pytest.mark.parametrize("name", list(MODULES))
def test_sharpen_reaches_the_floor(name):
    """sharpen_ on the module cases of tests/test_gpu_yolo11.py (same seeds, same input) reaches 0.2, and before it
    the softmax is near uniform -- the reason it exists."""
    from ydbl.utils.synthetic import trained_like_

    cls, args, c = MODULES[name]
    torch.manual_seed(0)
    o = trained_like_(getattr(U, cls)(*args).eval(), 0)
    x = torch.randn(2, c, 20, 20, generator=torch.Generator().manual_seed(11))
    before = U.attn_peaks(o, x)
    peaks = U.sharpen_(o, x)
    print(name, "peakedness before", before, "after", peaks)
    assert max(before) < 0.2 <= min(peaks)
