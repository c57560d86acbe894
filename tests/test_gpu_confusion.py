"""ydbl_confusion_matrix (device confusion matrix) against the CPU restatement of ConfusionMatrix.process_batch
(U/utils/metrics.py:326-382) in confusion_util.py: bit-equal counts, summed over the images of a batch.

Random scenes are checked to be tie-free first (a condition on the inputs: with no bit-equal participating IoUs the
reference's unspecified sort order cannot decide a cell), and every one must populate the diagonal, the
off-diagonal and both background lines, so that no case passes on an empty matrix.  The two no-GPU tests at the
end (descriptor layout, argument validation) need only the library."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from confusion_util import assert_not_trivial, assert_tie_free, confusion_reference, scene

gpu = pytest.mark.gpu
HEADER = Path(__file__).resolve().parent.parent / "include" / "ydbl.h"


def _run(det, cnt, boxes, cls, bidx, nc, conf=0.25, iou_thres=0.45, single_cls=False, cm=None):
    from ydbl.engine.validator import confusion_batch
    from ydbl.utils.metrics import ConfusionMatrix

    cm = cm or ConfusionMatrix(nc, conf=conf, iou_thres=iou_thres)
    confusion_batch(det.cuda(), cnt.cuda(), boxes, cls, bidx, cm, single_cls)
    return cm


# n, max_det, nc, single_cls, scene arguments
CASES = {
    "n4_det300_nc3": (4, 300, 3, False, {}),
    "nc80_empty_and_unlabelled": (3, 300, 80, False, {"empty_imgs": (1,), "no_label_imgs": (2,)}),
    "det1000_600_labels": (1, 1000, 3, False, {"labels": (600, 601)}),  # three LDS label chunks
    "nc100_global_counts": (2, 100, 100, False, {}),  # 101^2 cells: past the LDS-privatised counts
    "det1100_workspace_keys": (2, 1100, 3, False, {}),  # max_det past the LDS per-detection keys
    "single_cls": (3, 64, 3, True, {}),
    "one_label_chunk_edge": (2, 37, 5, False, {"labels": (256, 258)}),  # 256 / 257 labels: chunk boundary
}


@pytest.fixture(scope="module")
def scenes():
    """Each case's scene and its CPU reference, computed once and left unchanged."""
    out = {}
    for i, (name, (n, max_det, nc, single, kw)) in enumerate(CASES.items()):
        s = scene(n, max_det, nc, seed=100 + i, **kw)
        assert_tie_free(*s)
        ref = confusion_reference(*s, nc, single_cls=single)
        assert_not_trivial(ref, nc)
        out[name] = (s, ref)
    return out


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_confusion_bit_equal(scenes, name):
    n, max_det, nc, single, _ = CASES[name]
    (det, cnt, boxes, cls, bidx), ref = scenes[name]
    # labels arrive interleaved across images; the launcher groups them stably, and on tie-free inputs the
    # order of an image's labels decides nothing
    perm = torch.randperm(len(bidx), generator=torch.Generator().manual_seed(5))
    got = _run(det, cnt, boxes[perm], cls[perm], bidx[perm], nc, single_cls=single).matrix
    assert got.dtype == np.float64 and got.shape == (nc + 1, nc + 1)
    assert np.array_equal(got, ref), f"{int(np.abs(got - ref).sum())} counts differ"
    assert_not_trivial(got, nc)
    # columns of real classes count every label once (a matched label or a missed one)
    assert np.array_equal(got[:, :nc].sum(0), np.bincount(cls.int().numpy(), minlength=nc))


@gpu
def test_confusion_accumulates_and_repeats(scenes):
    from ydbl.utils.metrics import ConfusionMatrix

    (a, ref_a), (b, ref_b) = scenes["n4_det300_nc3"], scenes["single_cls"]
    cm = ConfusionMatrix(3)
    _run(*a, 3, cm=cm)
    _run(*b, 3, single_cls=True, cm=cm)
    assert np.array_equal(cm.matrix, ref_a + ref_b)  # two calls into one matrix == the two run separately
    assert np.array_equal(_run(*a, 3).matrix, ref_a)
    assert np.array_equal(_run(*a, 3).matrix, _run(*a, 3).matrix)  # the same call twice, fresh matrices


@gpu
def test_confusion_conf_is_strict():
    """A detection with confidence exactly 0.25 is not counted (detections[:, 4] > conf, :350)."""
    boxes = torch.tensor([[0.0, 0.0, 10.0, 10.0]])
    cls, bidx = torch.tensor([1.0]), torch.tensor([0])
    det = torch.zeros(1, 4, 6)
    det[0, 0] = torch.tensor([0.0, 0.0, 10.0, 10.0, 0.25, 1.0])
    det[0, 1] = torch.tensor([50.0, 50.0, 60.0, 60.0, 0.25, 2.0])
    cnt = torch.tensor([2], dtype=torch.int32)
    got = _run(det, cnt, boxes, cls, bidx, 3).matrix
    want = np.zeros((4, 4))
    want[3, 1] = 1  # the label is missed; neither detection appears
    assert np.array_equal(got, want) and np.array_equal(confusion_reference(det, cnt, boxes, cls, bidx, 3), want)
    det[0, :2, 4] = float(np.nextafter(np.float32(0.25), np.float32(1)))  # one fp32 step above: both count
    want = np.zeros((4, 4))
    want[1, 1] = want[2, 3] = 1
    assert np.array_equal(_run(det, cnt, boxes, cls, bidx, 3).matrix, want)
    # conf None / 0.001 (val's default) become 0.25 (:311)
    from ydbl.utils.metrics import ConfusionMatrix

    assert ConfusionMatrix(3, conf=0.001).conf == 0.25 and ConfusionMatrix(3, conf=None).conf == 0.25
    assert ConfusionMatrix(3, conf=0.5).conf == 0.5


@gpu
def test_confusion_exact_ties():
    """The two-label tie of test_match_exact_ties_larger_label with distinct classes: det0 has IoU exactly 0.6 with
    both labels, the larger label index takes it and label 0 is left to det1.  And one label, two identical
    detections: the larger detection index takes the label."""
    boxes = torch.tensor([[0.0, 0.0, 10.0, 10.0], [5.0, 0.0, 15.0, 10.0]])
    cls, bidx = torch.tensor([1.0, 2.0]), torch.tensor([0, 0])
    det = torch.zeros(1, 8, 6)
    det[0, 0] = torch.tensor([2.5, 0.0, 12.5, 10.0, 0.9, 0.0])
    det[0, 1] = torch.tensor([0.0, 0.0, 10.0, 10.0, 0.8, 1.0])
    cnt = torch.tensor([2], dtype=torch.int32)
    got = _run(det, cnt, boxes, cls, bidx, 3).matrix
    want = np.zeros((4, 4))
    want[0, 2] = 1  # det0 (class 0) -> label 1 (class 2)
    want[1, 1] = 1  # det1 (class 1) -> label 0 (class 1)
    assert np.array_equal(got, want)
    assert np.array_equal(confusion_reference(det, cnt, boxes, cls, bidx, 3), want)  # numpy's small-array order

    det[0, 0] = torch.tensor([0.0, 0.0, 10.0, 9.0, 0.9, 1.0])
    det[0, 1] = torch.tensor([0.0, 0.0, 10.0, 9.0, 0.8, 2.0])
    got = _run(det, cnt, boxes[:1], torch.tensor([0.0]), bidx[:1], 3).matrix
    want = np.zeros((4, 4))
    want[2, 0] = 1  # det1 wins the label
    want[1, 3] = 1  # det0 is a false positive
    assert np.array_equal(got, want)


@gpu
def test_confusion_many_ties(scenes):
    """A multi-label NMS keeps one box once per class, and labels can repeat: every second detection and every
    second label made a copy of its neighbour with another class, far more than 16 matches per image.  The
    reference's own order on these ties is unspecified there; with a stable argsort it is the documented rule."""
    (det, cnt, boxes, cls, bidx), _ = scenes["n4_det300_nc3"]
    det, boxes, cls = det.clone(), boxes.clone(), cls.clone()
    det[:, 1::2, :4] = det[:, 0:-1:2, :4]
    det[:, 1::2, 5] = (det[:, 0:-1:2, 5] + 1) % 3
    same = bidx[1::2] == bidx[0:-1:2][: len(bidx[1::2])]
    boxes[1::2][same] = boxes[0:-1:2][: len(same)][same]
    cls[1::2][same] = (cls[0:-1:2][: len(same)][same] + 2) % 3
    with pytest.raises(AssertionError):
        assert_tie_free(det, cnt, boxes, cls, bidx)
    ref = confusion_reference(det, cnt, boxes, cls, bidx, 3, kind="stable")
    assert_not_trivial(ref, 3)
    assert np.array_equal(_run(det, cnt, boxes, cls, bidx, 3).matrix, ref)


@gpu
def test_confusion_process_batch_per_image(scenes):
    """The reference's per-image interface, detections=None included, sums to the batched launch."""
    from ydbl.utils.metrics import ConfusionMatrix

    (det, cnt, boxes, cls, bidx), ref = scenes["nc80_empty_and_unlabelled"]
    cm = ConfusionMatrix(80)
    for b in range(det.shape[0]):
        sel = bidx == b
        p = det[b, : cnt[b]].cuda() if cnt[b] else None
        cm.process_batch(p, boxes[sel].cuda(), cls[sel].cuda())
    assert np.array_equal(cm.matrix, ref)
    tp, fp = cm.tp_fp()
    assert np.array_equal(tp, ref.diagonal()[:-1]) and np.array_equal(fp, (ref.sum(1) - ref.diagonal())[:-1])


class _Guarded:
    """A ConfusionMatrix stand-in whose accumulator sits in the middle of a larger zeroed buffer."""

    PAD = 4096

    def __init__(self, nc):
        self.nc, self.conf, self.iou_thres = nc, 0.25, 0.45
        self.buf = torch.zeros(2 * self.PAD + (nc + 1) ** 2, dtype=torch.int64, device="cuda")
        self.invalid = torch.zeros(1, dtype=torch.int32, device="cuda")

    def buffers(self, device):
        return self.buf[self.PAD: self.PAD + (self.nc + 1) ** 2], self.invalid


@gpu
def test_confusion_out_of_range_class(scenes):
    """Classes outside [0, nc): the reference raises IndexError; the kernel skips those counts, stays inside the
    matrix and reports them, and reading .matrix raises."""
    nc = 3
    (det, cnt, boxes, cls, bidx), _ = scenes["n4_det300_nc3"]
    det, cls = det.clone(), cls.clone()
    det[0, 0:20:3, 5] = 5.0
    det[1, 1, 5] = -2.0
    det[2, 2, 5] = 3.0  # == nc: the background index is not a class
    det[3, 3, 5] = 1e9
    cls[0], cls[-1] = 40000.0, -7.0
    skipped = []
    ref = confusion_reference(det, cnt, boxes, cls, bidx, nc, skipped=skipped)
    assert len(skipped) > 4
    with pytest.raises(IndexError):
        confusion_reference(det, cnt, boxes, cls, bidx, nc)
    g = _Guarded(nc)
    _run(det, cnt, boxes, cls, bidx, nc, cm=g)
    assert int(g.invalid.item()) == len(skipped)
    buf = g.buf.cpu().numpy()
    assert not buf[: g.PAD].any() and not buf[-g.PAD:].any(), "a count landed outside the matrix"
    assert np.array_equal(buf[g.PAD: -g.PAD].reshape(nc + 1, nc + 1), ref)
    cm = _run(det, cnt, boxes, cls, bidx, nc)
    with pytest.raises(IndexError):
        cm.matrix


def test_confusion_desc_layout_matches_c(tmp_path):
    """ydbl_confusion_desc against gcc's sizeof / offsetof, as test_abi.py's test_struct_layout_matches_c does."""
    from ydbl import _lib

    st = _lib.ConfusionDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ydbl_confusion_desc));']
    lines += [f'printf("{f} %zu\\n", offsetof(ydbl_confusion_desc, {f}));' for f, _ in st._fields_]
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.split("\n") if line.strip())
    assert int(got["size"]) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def test_confusion_validation_without_gpu():
    from ydbl import _lib

    lib = _lib.lib
    assert lib.ydbl_confusion_matrix(None, None) == 1
    assert "null descriptor" in lib.ydbl_last_error().decode()
    d = _lib.ConfusionDesc()
    assert lib.ydbl_confusion_matrix(d, None) == 1
    assert "null buffer" in lib.ydbl_last_error().decode()
    with pytest.raises(_lib.YdblError):
        _lib.check(lib.ydbl_confusion_matrix(d, None), "ydbl_confusion_matrix")
    full = dict(det=64, det_count=64, n=2, max_det=300, gt_box=64, gt_cls=64, gt_ofs=64, n_gt=5, nc=3, conf=0.25,
                iou_thres=0.45, matrix=64, invalid=64, workspace=64)
    for change, msg in [({"n": 0}, "empty batch"), ({"max_det": (1 << 20) + 1}, "max_det"),
                        ({"gt_box": None}, "labels missing"), ({"n_gt": -1}, "labels missing"),
                        ({"nc": 0}, "nc must be"), ({"nc": 40000}, "nc must be"),
                        ({"iou_thres": -0.1}, "iou_thres"), ({"iou_thres": float("nan")}, "iou_thres"),
                        ({"workspace": 68}, "8-byte aligned"), ({"matrix": 68}, "8-byte aligned")]:
        assert lib.ydbl_confusion_matrix(_lib.ConfusionDesc(**{**full, **change}), None) == 1, change
        assert msg in lib.ydbl_last_error().decode(), change
    assert lib.ydbl_confusion_workspace(2, 300, 10) == 8 * 10 + 16  # per-label keys; detection keys are in LDS
    assert lib.ydbl_confusion_workspace(2, 1100, 10) == 8 * (10 + 2 * 1100) + 16
    assert lib.ydbl_confusion_workspace(-1, 300, 10) == -1
