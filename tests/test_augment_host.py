"""Test-time augmentation, the parts that need no GPU: pass shapes and anchor windows (augment_passes), the
argument checks of ydbl_scale_img and ydbl_detect_decode_aug through the C ABI, and the fp8 scope guard."""

import ctypes as C

import pytest

from augment_util import expected_passes


@pytest.mark.parametrize("hw", [(160, 160), (160, 224), (640, 640), (1280, 1280)])
def test_augment_passes_match_the_formulas(hw):
    from ydbl.engine.session import augment_passes

    got = augment_passes(*hw, [8.0, 16.0, 32.0])
    assert [tuple(r) for r in got] == expected_passes(*hw)
    # windows tile the merged anchor axis in pass order, without gaps
    pos = 0
    for _, _, (sh, sw), (hp, wp), A, lo, hi, base in got:
        assert base == pos and 0 <= lo < hi <= A and sh <= hp and sw <= wp and hp % 32 == 0 and wp % 32 == 0
        pos += hi - lo


def test_augment_passes_known_values():
    from ydbl.engine.session import augment_passes

    p = augment_passes(160, 224, [8, 16, 32])
    assert [r[3] for r in p] == [(160, 224), (160, 192), (128, 160)]
    assert [r[2] for r in p] == [(160, 224), (132, 185), (107, 150)]
    assert [r[6] - r[5] for r in p] == [700, 630, 100]
    assert [(r[0], r[1]) for r in p] == [(1.0, False), (0.83, True), (0.67, False)]
    assert p[0][5:] == (0, 700, 0) and p[1][5:] == (0, 630, 700) and p[2][5:] == (320, 420, 1330)
    q = augment_passes(640, 640, [8, 16, 32])
    assert q[1][3] == (544, 544) and q[2][3] == (448, 448)
    assert [r[6] - r[5] for r in q] == [8000, 6069, 980] and q[2][7] + 980 == 15049


def test_scale_img_rejects_bad_descriptors():
    from ydbl import _lib

    lib = _lib.lib
    assert lib.ydbl_scale_img(None, None) == 1
    assert "null descriptor" in lib.ydbl_last_error().decode()

    def desc(**kw):
        f = dict(x=64, n=1, c=3, h=64, w=96, sh=53, sw=79, hp=64, wp=96, flip=0, pad_value=0.447, y=128)
        f.update(kw)
        return _lib.ScaleImgDesc(**f)

    for bad, msg in ((dict(x=None), "null buffer"), (dict(y=None), "null buffer"), (dict(n=0), "positive"),
                     (dict(h=0), "positive"), (dict(w=-1), "positive"), (dict(sh=0), "positive"),
                     (dict(sw=0), "positive"), (dict(hp=0), "positive"), (dict(sh=65), "exceeds"),
                     (dict(sw=97), "exceeds")):
        assert lib.ydbl_scale_img(C.byref(desc(**bad)), None) == 1, bad
        assert msg in lib.ydbl_last_error().decode(), (bad, lib.ydbl_last_error())


def _decode_desc(_lib, h=4, w=4, nc=3):
    box = (_lib.View * 3)(*[_lib.View(256, 1, h, w, 64, 72, _lib.F32)] * 3)
    cls = (_lib.View * 3)(*[_lib.View(512, 1, h, w, nc, 72, _lib.F32)] * 3)
    strides = (C.c_float * 3)(8.0, 16.0, 32.0)
    return _lib.DecodeDesc(box, cls, 1, nc, strides, 0.25, 0, None, 0, None, 1024, 1024, 1024, 1024, 1024, 64)


def test_decode_aug_rejects_bad_records():
    from ydbl import _lib

    lib = _lib.lib
    d = _decode_desc(_lib)  # one 4x4 level: 16 anchors
    assert lib.ydbl_detect_decode_aug(C.byref(d), None, None) == 1
    assert "null augmentation record" in lib.ydbl_last_error().decode()
    assert lib.ydbl_detect_decode_aug(None, C.byref(_lib.DecodeAug()), None) == 1
    for bad in (dict(scale=-1.0), dict(scale=float("nan")), dict(flip_w=float("inf")), dict(a_lo=-1),
                dict(a_lo=4, a_hi=4), dict(a_lo=8, a_hi=4), dict(a_hi=17), dict(pos_base=-1),
                dict(a_lo=0, a_hi=16, pos_base=10, y_stride=20), dict(y_stride=8)):
        g = _lib.DecodeAug(**bad)
        assert lib.ydbl_detect_decode_aug(C.byref(d), C.byref(g), None) == 1, bad
        assert "decode_aug" in lib.ydbl_last_error().decode(), (bad, lib.ydbl_last_error())
    # the plain descriptor's own checks still apply
    d.cap = 0
    assert lib.ydbl_detect_decode_aug(C.byref(d), C.byref(_lib.DecodeAug()), None) == 1
    assert "candidate buffers" in lib.ydbl_last_error().decode()


def test_decode_aug_layout_matches_c(tmp_path):
    """The two new descriptors against gcc's sizeof / offsetof, as tests/test_abi.py checks the others."""
    import subprocess
    from pathlib import Path

    from ydbl import _lib

    header = Path(__file__).resolve().parent.parent / "include" / "ydbl.h"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    structs = {"ydbl_decode_aug": _lib.DecodeAug, "ydbl_scale_img_desc": _lib.ScaleImgDesc}
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.split("\n") if line.strip())
    for cname, st in structs.items():
        assert int(got[cname]) == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(st, fname).offset, f"{cname}.{fname}"


def test_augment_with_fp8_hits_the_scope_guard():
    import torch

    from ydbl import YOLO

    p = YOLO("yolov13n_DBL.yaml", nc=3)
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="augment"):
        p.predict(x, augment=True, fp8=True, half=True)
    with pytest.raises(NotImplementedError, match="augment"):
        p.session(1, 64, 64, half=True, fp8=True, augment=True)
    with pytest.raises(NotImplementedError, match="augment"):
        p.val([{"img": x}], augment=True, fp8=True)
    assert p.overrides.get("augment") is None  # nothing sticks
