"""The segmentation models (yolo11-seg.yaml / yolov8-seg.yaml: Segment in place of Detect) on the host: construction
from tests/golden/yolo11-seg.json / yolov8-seg.json, the parser's scaling of the proto width, reference parameter
names and shapes, the YAML route, the task, the guards raised before a device is touched, the Masks / Results
containers, the two new descriptors' layouts -- and the condition on the mask test inputs under which the GPU tests
compare masks (tests/seg_util.py: the near-zero set is small, and the restatement's own fp32 leg agrees with its fp64
leg everywhere outside it).  No GPU."""

import ctypes as C
import json
import subprocess
from pathlib import Path

import pytest
import torch

import seg_util as S

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ydbl.h"
FAMS = ["yolo11", "yolov8"]


@pytest.mark.parametrize("family", FAMS)
def test_layer_list_scaling_and_task(family, golden_dir):
    from ydbl import YOLO
    from ydbl.nn import modules as M

    ref = json.loads((golden_dir / f"{family}.json").read_text())
    seg = json.loads((golden_dir / f"{family}-seg.json").read_text())
    assert seg["backbone"] == ref["backbone"] and seg["head"][:-1] == ref["head"][:-1]
    assert seg["scales"] == ref["scales"]
    assert seg["head"][-1] == [ref["head"][-1][0], 1, "Segment", ["nc", 32, 256]]
    p = YOLO(str(golden_dir / f"{family}n-seg.json"), nc=3)
    d = YOLO(str(golden_dir / f"{family}n.json"), nc=3)
    assert p.task == "segment" and d.task == "detect"
    assert [type(m).__name__ for m in p.model.model[:-1]] == [type(m).__name__ for m in d.model.model[:-1]]
    head = p.model.model[-1]
    assert type(head) is M.Segment and isinstance(head, M.Detect) and type(head.proto) is M.Proto
    assert (head.nm, head.npr, head.nc) == (32, 64, 3)  # 256 * width 0.25
    assert head.proto.upsample.in_channels == head.proto.upsample.out_channels == 64
    assert all(seq[0].conv.out_channels == 32 and seq[2].out_channels == 32 for seq in head.cv4)  # c4 = max(64//4, 32)
    assert head.legacy is S.FAMILIES[family]
    assert p.model.stride.tolist() == [8.0, 16.0, 32.0]
    cm = p.model.compile(2, 64, 64, torch.float16, device="meta")  # shape-only plan
    assert [lv.shape for lv in cm.levels] == [(2, 8, 8, 67), (2, 4, 4, 67), (2, 2, 2, 67)]  # Detect's layout, untouched
    proto, mcs = cm.plan.seg
    assert proto.shape == (2, 16, 16, 32) and [v.shape for v in mcs] == [(2, 8, 8, 32), (2, 4, 4, 32), (2, 2, 2, 32)]
    assert sum(st.what == "deconv2x2" for st in cm.plan.steps) == 1
    s = YOLO(str(golden_dir / f"{family}s-seg.json"), nc=3).model.model[-1]
    assert s.npr == 128 and s.cv4[0][0].conv.out_channels == 32


@pytest.mark.parametrize("family", FAMS)
def test_state_dict_matches_the_restatement(family, golden_dir):
    from ydbl import YOLO

    p = YOLO(str(golden_dir / f"{family}n-seg.json"), nc=3)
    o = S.build_oracle(family, "n", 3)
    sp, so = p.model.state_dict(), o.state_dict()
    assert list(sp) == list(so)
    assert all(sp[k].shape == so[k].shape for k in so)
    assert any(k.endswith("proto.upsample.weight") for k in sp) and any(".cv4.2.2.bias" in k for k in sp)
    p.model.load_state_dict(so, strict=True)
    o.load_state_dict(p.model.state_dict(), strict=True)


def test_yaml_name_resolves_to_the_unified_file(tmp_path, golden_dir):
    import yaml

    from ydbl import YOLO

    d = json.loads((golden_dir / "yolo11-seg.json").read_text())
    (tmp_path / "yolo11-seg.yaml").write_text(yaml.safe_dump(d, default_flow_style=None).replace("null", "None"))
    a = YOLO(str(tmp_path / "yolo11n-seg.yaml"), nc=3)
    b = YOLO(str(golden_dir / "yolo11n-seg.json"), nc=3)
    assert a.task == "segment" and a.model.yaml["scale"] == "n"
    assert [(k, tuple(v.shape)) for k, v in a.model.state_dict().items()] == [
        (k, tuple(v.shape)) for k, v in b.model.state_dict().items()]


def test_guards_raise_before_a_device_is_touched(golden_dir):
    """fp8, the loss and the batch-sharded predictor: NotImplementedError from the host checks (there is no GPU here:
    anything that reached for a device would raise something else)."""
    from ydbl import YOLO
    from ydbl.engine.session import DetectSession
    from ydbl.parallel import ShardedPredictor

    p = YOLO(str(golden_dir / "yolo11n-seg.json"), nc=3)
    with pytest.raises(NotImplementedError, match="fp8"):
        p.session(1, 64, 64, fp8=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        DetectSession(p.model, 1, 64, 64, torch.float16, fp8=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        p.predict(torch.zeros(1, 3, 64, 64), fp8=True)
    with pytest.raises(NotImplementedError, match="v8SegmentationLoss"):
        p.session(1, 64, 64, loss=True)
    with pytest.raises(NotImplementedError, match="v8SegmentationLoss"):
        p.model.loss({"img": torch.zeros(1, 3, 64, 64), "batch_idx": torch.zeros(0), "cls": torch.zeros(0, 1),
                      "bboxes": torch.zeros(0, 4)})
    with pytest.raises(NotImplementedError, match="v8SegmentationLoss"):
        p.model.init_criterion()
    with pytest.raises(NotImplementedError, match="v8SegmentationLoss"):
        p.val([], loss=True)
    with pytest.raises(NotImplementedError, match="batch-sharded"):
        ShardedPredictor(p, 4, 64, 64, device=0)
    with pytest.raises(ValueError, match="mask_dtype"):
        p.predict(torch.zeros(1, 3, 64, 64), mask_dtype=torch.float16)


def test_masks_and_results_containers():
    from ydbl.engine.results import Masks, Results

    data = (torch.arange(3 * 4 * 5).reshape(3, 4, 5) % 2).float()
    m = Masks(data, (8, 10))
    assert len(m) == 3 and m.shape == (3, 4, 5) and m.orig_shape == (8, 10)
    assert torch.equal(m[1].data, data[1:2]) and m[1].shape == (1, 4, 5)
    assert torch.equal(m[[0, 2]].data, data[[0, 2]])
    assert isinstance(m.numpy().data, __import__("numpy").ndarray) and m.cpu().data.device.type == "cpu"
    assert m.to(torch.uint8).data.dtype == torch.uint8
    for name in ("xy", "xyn"):
        with pytest.raises(NotImplementedError, match="contour"):
            getattr(m, name)
    boxes = torch.tensor([[0, 0, 4, 4, 0.9, 0], [1, 1, 5, 5, 0.8, 1], [2, 2, 6, 6, 0.7, 2.0]])
    r = Results(torch.zeros(8, 10, 3), "a.jpg", {0: "a", 1: "b", 2: "c"}, boxes=boxes, masks=lambda: data)
    assert len(r) == 3 and len(r.masks) == 3 and r.masks.orig_shape == (8, 10)
    sub = r[1:]
    assert len(sub.boxes) == 2 and torch.equal(sub.masks.data, data[1:])
    assert r.cpu().masks.data.shape == (3, 4, 5) and r.numpy().masks.data.shape == (3, 4, 5)
    assert r.new().masks is None
    r2 = r.new()
    r2.update(boxes=boxes[:1].clone(), masks=data[:1])
    assert len(r2.masks) == 1 and len(r2.boxes) == 1
    empty = Results(torch.zeros(8, 10, 3), "b.jpg", {0: "a"}, boxes=torch.zeros(0, 6), masks=lambda: None)
    assert empty.masks is None and len(empty) == 0 and empty[0:0].masks is None
    assert empty.summary() == []
    for call in (lambda: r.summary(), lambda: r.save_txt("unused.txt"), lambda: r.plot()):
        with pytest.raises(NotImplementedError):
            call()
    assert r.plot(masks=False).shape == (8, 10, 3)


def test_new_descriptors_match_c(tmp_path):
    """The ctypes mirrors of ydbl_deconv_desc and ydbl_mask_desc against gcc's sizeof / offsetof (test_abi's method)."""
    from ydbl import _lib

    structs = {"ydbl_deconv_desc": "DeconvDesc", "ydbl_mask_desc": "MaskDesc", "ydbl_nms_desc": "NmsDesc"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, pyname in structs.items():
        lines.append(f'printf("{pyname} %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'printf("{pyname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split() for line in out if line.strip())
    for pyname in structs.values():
        st = getattr(_lib, pyname)
        assert int(got[pyname]) == C.sizeof(st), pyname
        for fname, _ in st._fields_:
            assert int(got[f"{pyname}.{fname}"]) == getattr(st, fname).offset, f"{pyname}.{fname}"
    assert _lib.NmsDesc._fields_[-1][0] == "out_idx"


def test_new_entry_points_refuse_bad_descriptors():
    from ydbl import _lib

    lib = _lib.lib
    assert lib.ydbl_deconv2x2_nhwc(None, None) == 1
    d = _lib.DeconvDesc()
    d.x = _lib.View(16, 1, 4, 4, 48, 48, _lib.F16)  # 48 is no multiple of 32
    d.y = _lib.View(4096, 1, 8, 8, 64, 64, _lib.F16)
    d.w = 8192
    assert lib.ydbl_deconv2x2_nhwc(d, None) == 1 and "multiples of 32" in lib.ydbl_last_error().decode()
    d.x = _lib.View(16, 1, 4, 4, 64, 64, _lib.F16)
    d.y = _lib.View(4096, 1, 8, 9, 64, 64, _lib.F16)
    assert lib.ydbl_deconv2x2_nhwc(d, None) == 1 and "2h, 2w" in lib.ydbl_last_error().decode()
    assert lib.ydbl_process_mask(None, None) == 1
    m = _lib.MaskDesc()
    m.proto = _lib.View(16, 1, 4, 4, 12, 16, _lib.F32)  # nm 12
    assert lib.ydbl_process_mask(m, None) == 1 and "multiple of 8" in lib.ydbl_last_error().decode()
    m.proto = _lib.View(16, 1, 4, 4, 72, 72, _lib.F32)
    assert lib.ydbl_process_mask(m, None) == 1 and "at most 64" in lib.ydbl_last_error().decode()
    m.proto = _lib.View(16, 1, 4, 4, 32, 32, _lib.F32)
    m.max_det = 5000
    assert lib.ydbl_process_mask(m, None) == 1 and "max_det" in lib.ydbl_last_error().decode()


def test_mask_window_is_scale_masks_crop():
    from ydbl.utils.ops import mask_window

    for mh, mw, shape in [(24, 40, (75, 150)), (24, 40, (101, 127)), (16, 16, (200, 173)), (160, 160, (480, 640))]:
        top, left, bottom, right = mask_window(mh, mw, shape)
        x = torch.arange(mh * mw, dtype=torch.float32).reshape(1, 1, mh, mw)
        want = S.scale_masks(x, shape)
        got = torch.nn.functional.interpolate(x[..., top:bottom, left:right], shape, mode="bilinear",
                                              align_corners=False)
        assert torch.equal(got, want)


@pytest.mark.parametrize("form,mh,mw,shape", S.MASK_FORMS)
def test_condition_on_the_mask_inputs(form, mh, mw, shape):
    """Seeds 0-3, N(0, 1) prototypes (fp32 and rounded to fp16) and coefficients, nm 32 and 8, the seven boxes: the
    near-zero set |v64| <= 2^-16 S holds at most 0.1 % of the S > 0 pixels, and the restatement's fp32 leg agrees with
    its fp64 leg on every pixel outside it (S == 0 pixels included: exactly 0)."""
    frame = shape if form == "native" else (4 * mh, 4 * mw)
    boxes = S.mask_boxes(*frame)
    near_tot = pos_tot = 0
    for seed in range(4):
        for nm, half in ((32, False), (32, True), (8, False)):
            proto, coef = S.mask_inputs(seed, mh, mw, nm, half)
            v64, s64 = S.mask_reference(form, proto, coef, boxes, (7, 1), frame)
            leg = S.mask_leg32(form, proto, coef, boxes, (7, 1), frame)
            for g, v, s in zip(leg, v64, s64):
                wrong, near, pos = S.mask_check(g, v, s)
                assert wrong == 0
                assert near <= S.NEAR_ZERO_CAP * pos
                near_tot += near
                pos_tot += pos
    assert pos_tot > 0
    print(f"near-zero share {form} {mh}x{mw} -> {shape}: {near_tot} / {pos_tot} = {near_tot / pos_tot:.2e}")
