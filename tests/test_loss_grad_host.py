"""The loss gradient without a GPU: the given-assignment restatement (tests/loss_grad_util.py) reproduces the three loss
terms of tests/loss_util.reference_loss when fed that function's own assignment, the ctypes mirror of
ydbl_loss_grad_desc has the C layout (gcc's sizeof / offsetof, as tests/test_abi.py), and ydbl_detect_loss_grad
rejects bad arguments before anything is launched."""

import ctypes as C
import subprocess
from pathlib import Path

import pytest
import torch

from loss_grad_util import given_assignment_grads, given_assignment_loss
from loss_util import flatten_levels, reference_loss, rel_dist, synthetic_case

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ydbl.h"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_terms_equal_the_full_restatement_in_fp64(seed):
    levels, shapes, strides, gt = synthetic_case(seed)
    box, cls = flatten_levels(levels)
    r = reference_loss(box, cls, shapes, strides, gt, dtype=torch.float64)
    assert int(r["fg"].sum()) > 0
    total, terms = given_assignment_loss(box, cls, shapes, strides, gt, r["fg"], r["target_gt_idx"],
                                         r["target_score"], r["target_scores_sum"], dtype=torch.float64)
    for j in range(3):
        assert rel_dist(terms[j], r["loss"][j]) <= 1e-12, (j, float(terms[j]), float(r["loss"][j]))
    assert rel_dist(total, r["loss"].sum() * box.shape[0]) <= 1e-12


def test_gradient_structure_on_the_cpu():
    """Non-foreground anchors get no box gradient, and without labels the class gradient is K * gain_cls * sigmoid."""
    levels, shapes, strides, gt = synthetic_case(0)
    box, cls = flatten_levels(levels)
    r = reference_loss(box, cls, shapes, strides, gt, dtype=torch.float64)
    gb, gc, _ = given_assignment_grads(box, cls, shapes, strides, gt, r["fg"], r["target_gt_idx"], r["target_score"],
                                       r["target_scores_sum"])
    assert float(gb[~r["fg"]].abs().max()) == 0.0 and float(gb[r["fg"]].abs().max()) > 0.0
    z = torch.zeros(box.shape[:2])
    gb, gc, _ = given_assignment_grads(box, cls, shapes, strides, torch.zeros_like(gt), z.bool(), z.long(), z, 1.0)
    assert float(gb.abs().max()) == 0.0
    assert rel_dist(gc, box.shape[0] * 0.5 * cls.double().sigmoid()) <= 1e-12


def test_loss_grad_desc_layout_matches_c(tmp_path):
    from ydbl import _lib

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ydbl_loss_grad_desc));']
    for fname, _ in _lib.LossGradDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(ydbl_loss_grad_desc, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.splitlines() if line.strip())
    assert int(got["size"]) == C.sizeof(_lib.LossGradDesc)
    for fname, _ in _lib.LossGradDesc._fields_:
        assert int(got[fname]) == getattr(_lib.LossGradDesc, fname).offset, fname


def _desc():
    """A descriptor whose every field passes validation (the pointers are never followed on the host)."""
    from ydbl import _lib

    d = _lib.LossGradDesc()
    d.nl, d.nc, d.reg_max, d.max_labels = 3, 3, 16, 6
    d.gain_box, d.gain_cls, d.gain_dfl, d.batch_scale = 7.5, 0.5, 1.5, 2.0
    d.gt = d.fg = d.target_gt_idx = d.target_score = d.target_scores_sum = 4096
    for i, (h, w, s) in enumerate(((8, 12, 8.0), (4, 6, 16.0), (2, 3, 32.0))):
        d.box[i] = _lib.View(4096, 2, h, w, 64, 67, _lib.F16)
        d.cls[i] = _lib.View(4096 + 128, 2, h, w, 3, 67, _lib.F16)
        d.gbox[i] = _lib.View(8192, 2, h, w, 64, 72, _lib.F32)
        d.gcls[i] = _lib.View(8192 + 256, 2, h, w, 3, 72, _lib.F32)
        d.stride[i] = s
    return d


def test_loss_grad_validation_errors_without_gpu():
    from ydbl import _lib

    lib = _lib.lib

    def err(d):
        rc = lib.ydbl_detect_loss_grad(d, None)
        return rc, lib.ydbl_last_error().decode()

    rc, msg = err(None)
    assert rc == 1 and "null descriptor" in msg
    d = _desc()
    d.gbox[1].ptr = None
    rc, msg = err(d)
    assert rc == 1 and "null gradient view" in msg
    d = _desc()
    d.gcls[2].ptr = None
    rc, msg = err(d)
    assert rc == 1 and "null gradient view" in msg
    d = _desc()
    d.reg_max = 8
    rc, msg = err(d)
    assert rc == 1 and "reg_max" in msg
    d = _desc()
    d.nl = 0
    rc, msg = err(d)
    assert rc == 1 and "nl" in msg
    for field, value in (("w", 7), ("h", 9), ("n", 3), ("c", 63), ("cs", 60)):
        d = _desc()
        setattr(d.gbox[0], field, value)
        rc, msg = err(d)
        assert rc == 1 and "gradient view shapes" in msg, (field, msg)
    d = _desc()
    d.gcls[1].c = 4
    rc, msg = err(d)
    assert rc == 1 and "gradient view shapes" in msg
    d = _desc()
    d.target_score = None
    rc, msg = err(d)
    assert rc == 1 and "null buffer" in msg
    d = _desc()
    d.gbox[0].dtype = 7
    rc, msg = err(d)
    assert rc == 1 and "dtype" in msg
