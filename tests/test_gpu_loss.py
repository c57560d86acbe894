"""ydbl_detect_loss on the device against the CPU restatement of the reference's loss (tests/loss_util.py), on
synthetic level maps -- no model.  Shapes are the smallest that exercise every branch: three levels, A = 126 (one
workgroup) and A = 315 (two), nc = 3 and 80, fp32 and fp16 levels, an image without labels, labels with fewer than ten
in-box anchors, anchors selected by two labels, a duplicated label, a label that contains no anchor centre, and one
544 x 544 image under a box with more in-box cells per select thread than the keys it keeps.

Every case first asserts, on the CPU, that its inputs are decidable: every label's 10th / 11th metric gap is > 1e-3,
at least one anchor is selected by two labels, at least one label has fewer than ten in-box anchors, and the fp32 and
fp64 restatements assign identically.  A case that does not meet them fails.

Tolerance: the yardstick of a quantity (the three losses, the per-image table, the target scores) is the fp32
restatement's own relative distance to the fp64 restatement on the same inputs, the largest over this file's cases;
the kernel, whose reduction order over 10^3..10^5 terms and whose exp / log / atan differ from the CPU's in the last
bits, gets 32 x that against the fp64 restatement (target_scores_sum: the losses' yardstick).  Distances seen on the
MI355X: profiles/r18/r18_loss_parity.txt (at most 1.0e-6 against bounds of 2.0e-5 .. 4.6e-5).
"""

import pytest
import torch

from loss_util import GAINS, flatten_levels, reference_loss, rel_dist, synthetic_case

pytestmark = pytest.mark.gpu

FACTOR = 32.0


def table_dist(a, b):
    """Largest column-wise relative distance of two [rows, 3] tables (a column: one of box / cls / dfl)."""
    a, b = torch.as_tensor(a).double().reshape(-1, 3), torch.as_tensor(b).double().reshape(-1, 3)
    return max(rel_dist(a[:, j], b[:, j]) for j in range(3))


def special_case():
    """Base seed 0 with image 1's label 1 replaced by a copy of its label 0 and its label 2 by a 2 x 2 px box that
    holds no anchor centre on any level (centres sit at multiples of 4 px)."""
    levels, shapes, strides, gt = synthetic_case(0)
    gt = gt.clone()
    gt[1, 1] = gt[1, 0]
    gt[1, 2] = torch.tensor([1.0, 1.0, 1.0, 3.0, 3.0])
    return levels, shapes, strides, gt


def full_box_case():
    """One 544 x 544 image (A = 6069, 24 workgroups) whose first two labels are the same box over nearly the whole
    input: 5933 in-box anchors, so a select thread walks up to 19 + 5 + 2 cells -- more than the 16 keys it keeps --
    and every pick of the pair is a double pick.  The third label holds 7 anchor centres."""
    levels, shapes, strides, _ = synthetic_case(0, h=544, w=544, counts=(1,), max_labels=4)
    gt = torch.zeros(1, 4, 5)
    gt[0, 0] = torch.tensor([1.0, 3.0, 5.0, 541.0, 539.0])
    gt[0, 1] = gt[0, 0]
    gt[0, 2] = torch.tensor([2.0, 100.0, 200.0, 121.0, 219.0])
    return levels, shapes, strides, gt


def build_cases():
    cases = {}
    for seed in range(6):
        cases[f"base-{seed}"] = (synthetic_case(seed), torch.float32)
        cases[f"half-{seed}"] = (synthetic_case(seed), torch.float16)
    cases["nc80"] = (synthetic_case(1, nc=80), torch.float32)
    cases["96x160"] = (synthetic_case(5, h=96, w=160), torch.float32)
    cases["special"] = (special_case(), torch.float32)
    cases["544-full-box"] = (full_box_case(), torch.float32)
    return cases


class Case:
    def __init__(self, name, inputs, dtype):
        levels, self.shapes, self.strides, self.gt = inputs
        self.name, self.dtype = name, dtype
        self.levels = [lv.to(dtype) for lv in levels]  # what the device reads; the restatement gets the same values
        box, cls = flatten_levels([lv.float() for lv in self.levels])
        self.nc = cls.shape[-1]
        self.r32 = reference_loss(box, cls, self.shapes, self.strides, self.gt, dtype=torch.float32)
        self.r64 = reference_loss(box, cls, self.shapes, self.strides, self.gt, dtype=torch.float64)
        self.yard = {"loss": table_dist(self.r32["loss"], self.r64["loss"]),
                     "per_image": table_dist(self.r32["per_image"], self.r64["per_image"]),
                     "target_score": rel_dist(self.r32["target_score"], self.r64["target_score"])}


@pytest.fixture(scope="module")
def cases():
    """The references, computed once and left unchanged."""
    return {k: Case(k, inp, dt) for k, (inp, dt) in build_cases().items()}


@pytest.fixture(scope="module")
def yardstick(cases):
    y = {k: max(c.yard[k] for c in cases.values()) for k in ("loss", "per_image", "target_score")}
    y["target_scores_sum"] = y["loss"]
    return y


def run_device(case, debug=True, pad=0):
    """One ydbl_detect_loss launch over the case's levels as [B, h, w, 64+nc(+pad)] device buffers read in place."""
    from ydbl import _lib
    from ydbl.utils.loss import LossBuffers

    dev = torch.device("cuda", 0)
    keep, boxes, clss = [], [], []
    for lv in case.levels:
        B, h, w, c = lv.shape
        buf = torch.full((B, h, w, c + pad), float("nan"), dtype=case.dtype, device=dev)  # (a read of the pad shows)
        buf[..., :c] = lv.to(dev)
        keep.append(buf)
        dt, es = _lib.dtype_code(case.dtype), buf.element_size()
        boxes.append(_lib.View(buf.data_ptr(), B, h, w, 64, c + pad, dt))
        clss.append(_lib.View(buf.data_ptr() + 64 * es, B, h, w, c - 64, c + pad, dt))
    bufs = LossBuffers(boxes, clss, case.strides, case.nc, GAINS, case.gt.shape[1], 10, dev, debug=debug)
    bufs.gt.copy_(case.gt)
    bufs.launch()
    torch.cuda.synchronize(dev)
    return bufs, keep


def check_conditions(c):
    assert c.r64["gaps"] and min(c.r64["gaps"]) > 1e-3, (c.name, min(c.r64["gaps"], default=None))
    assert min(c.r32["gaps"]) > 1e-3, (c.name, min(c.r32["gaps"]))
    assert c.r64["multi_selected"] >= 1, c.name
    assert c.r64["short_labels"] >= 1, c.name
    assert torch.equal(c.r32["fg"], c.r64["fg"]), c.name
    assert torch.equal(c.r32["target_gt_idx"], c.r64["target_gt_idx"]), c.name


def check_device(c, bufs, bound):
    r = c.r64
    fg, tgi = bufs.fg.cpu().bool(), bufs.target_gt_idx.cpu().long()
    sure = r["target_score"] > 0  # elsewhere the reference's zero-metric picks are unspecified (include/ydbl.h)
    assert torch.equal(fg[sure], r["fg"][sure])
    assert torch.equal(tgi[sure], r["target_gt_idx"][sure])
    assert not bool(fg[~r["fg"]].any())  # the kernel never makes an anchor fg that the reference does not
    d = {"target_score": rel_dist(bufs.target_score.cpu(), r["target_score"]),
         "loss": table_dist(bufs.loss.cpu(), r["loss"]),
         "per_image": table_dist(bufs.per_image.cpu(), r["per_image"]),
         "target_scores_sum": rel_dist(bufs.target_scores_sum.cpu(), r["target_scores_sum"])}
    print(f"{c.name}: " + " ".join(f"{k} {v:.3g} (bound {bound[k]:.3g})" for k, v in d.items())
          + f" | fg {int(r['fg'].sum())} multi {r['multi_selected']} short {r['short_labels']}"
          + f" gap {min(r['gaps']):.3g} loss {[float(v) for v in bufs.loss.cpu()]}")
    for k, v in d.items():
        assert v <= bound[k], (c.name, k, v, bound[k])
    rows = bufs.per_image.cpu().double().sum(0)
    assert table_dist(rows, bufs.loss.cpu()) <= bound["per_image"]  # the rows add up to the total
    return d


NAMES = sorted(build_cases())


@pytest.mark.parametrize("name", NAMES)
def test_loss_matches_restatement(cases, yardstick, name):
    c = cases[name]
    check_conditions(c)
    bufs, _ = run_device(c)
    check_device(c, bufs, {k: FACTOR * v for k, v in yardstick.items()})


def test_special_case_semantics(cases, yardstick):
    c = cases["special"]
    r = c.r64
    # on the CPU first: the duplicate's anchors all go to the lower index, the empty box gets none
    assert int((r["fg"][1] & (r["target_gt_idx"][1] == 0)).sum()) > 0
    assert int((r["fg"][1] & (r["target_gt_idx"][1] == 1)).sum()) == 0
    assert int((r["fg"][1] & (r["target_gt_idx"][1] == 2)).sum()) == 0
    assert r["in_box"][6 + 2] == 0  # image 1's third label (labels listed image by image: 6 of image 0 first)
    bufs, _ = run_device(c)
    fg, tgi = bufs.fg.cpu().bool(), bufs.target_gt_idx.cpu()
    assert int((fg[1] & (tgi[1] == 0)).sum()) == int((r["fg"][1] & (r["target_gt_idx"][1] == 0) &
                                                       (r["target_score"][1] > 0)).sum())
    assert int((fg[1] & (tgi[1] == 1)).sum()) == 0 and int((fg[1] & (tgi[1] == 2)).sum()) == 0
    assert not bool(fg[2].any())  # the image without labels
    assert float(bufs.per_image[2, 0]) == 0.0 and float(bufs.per_image[2, 2]) == 0.0 and float(bufs.per_image[2, 1]) > 0


def test_no_labels_at_all(cases, yardstick):
    """Nothing is fg: loss[0] and loss[2] stay 0, the class term is BCE against zeros over max(sum, 1) = 1."""
    base = cases["base-0"]
    c = Case("empty", (base.levels, base.shapes, base.strides, torch.zeros_like(base.gt)), torch.float32)
    bufs, _ = run_device(c)
    assert float(bufs.loss[0]) == 0.0 and float(bufs.loss[2]) == 0.0
    assert float(bufs.target_scores_sum) == 1.0
    assert table_dist(bufs.loss.cpu(), c.r64["loss"]) <= FACTOR * yardstick["loss"]
    assert not bool(bufs.fg.any())


def test_bit_identical_and_pitch_independent(cases):
    """Two launches on the same inputs give the same bits, and so does a wider channel pitch (the pad is never read:
    it holds NaN) and a run without the optional assignment outputs."""
    c = cases["base-3"]
    a, _ = run_device(c)
    b, _ = run_device(c)
    for x, y in ((a.out, b.out), (a.fg, b.fg), (a.target_gt_idx, b.target_gt_idx), (a.target_score, b.target_score)):
        assert torch.equal(x.cpu(), y.cpu())
    p, _ = run_device(c, pad=5)
    assert torch.equal(a.out.cpu(), p.out.cpu()) and torch.equal(a.target_score.cpu(), p.target_score.cpu())
    q, _ = run_device(c, debug=False)
    assert torch.equal(a.out.cpu(), q.out.cpu())
    h = cases["half-3"]
    a, _ = run_device(h)
    p, _ = run_device(h, pad=3)  # odd pitch: 2-byte aligned pixels only
    assert torch.equal(a.out.cpu(), p.out.cpu())
