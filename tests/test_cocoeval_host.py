"""The host side of val(coco_eval=True), no GPU: coco_accumulate / coco_summarize (ydbl.utils.metrics) against the
numpy restatement of the COCO protocol in cocoeval_util.py on restatement-made flags, the three worked cases of the
protocol, the ABI of ydbl_coco_match (validation paths only, nothing is launched), and a check that the scenes the GPU
tests run are not trivial."""

import ctypes as C
import inspect
import subprocess
from pathlib import Path

import numpy as np
import pytest

import cocoeval_util as U
from ydbl import _lib
from ydbl.utils.metrics import (COCO_AREA_RNG, COCO_IOU_THRS, COCO_MAX_DETS, COCO_REC_THRS, COCO_STAT_NAMES,
                                DetMetrics, coco_accumulate, coco_summarize, coco_summary_lines)

HEADER = Path(__file__).resolve().parent.parent / "include" / "ydbl.h"
TOL = 1e-12  # values in [0, 1], both sides fp64 sums of at most a few thousand terms


def batch_of(labels, dets, classes=None):
    """One image from xywh labels and (x, y, w, h, score[, class]) detections."""
    det = np.zeros((1, max(len(dets), 1), 6), np.float32)
    for i, d in enumerate(dets):
        det[0, i] = [d[0], d[1], d[0] + d[2], d[1] + d[3], d[4], d[5] if len(d) > 5 else 0]
    boxes = np.array([[x, y, x + w, y + h] for x, y, w, h in labels], np.float32).reshape(-1, 4)
    cls = np.zeros(len(labels), np.float32) if classes is None else np.array(classes, np.float32)
    return det, np.array([len(dets)], np.int32), boxes, cls, np.zeros(len(labels), np.int64)


def both(batches, nc, single=False):
    """(restatement stats, product stats, restatement eval, product eval, per-image dicts) on restatement flags."""
    arrays, imgs, ev, stats = U.run(batches, nc, single)
    recs = [U.product_record(b[0], a, b[3], b[4], nc, single) for b, a in zip(batches, arrays)]
    pev = coco_accumulate(recs, nc)
    return stats, coco_summarize(pev), ev, pev, imgs


def assert_same(ev, pev, stats, pstats):
    assert pstats.dtype == np.float64 and pstats.shape == (12,)
    assert np.abs(pstats - stats).max() <= TOL
    for key in ("precision", "recall", "scores"):
        assert pev[key].shape == ev[key].shape and pev[key].dtype == np.float64
        assert np.abs(pev[key] - ev[key]).max() <= TOL, key


def test_params_are_the_protocols():
    assert np.array_equal(COCO_IOU_THRS, np.linspace(0.5, 0.95, 10)) and COCO_IOU_THRS.dtype == np.float64
    assert np.array_equal(COCO_REC_THRS, np.linspace(0, 1, 101))
    assert list(COCO_MAX_DETS) == [1, 10, 100]
    assert [list(r) for r in COCO_AREA_RNG] == [[0, 1e10], [0, 32**2], [32**2, 96**2], [96**2, 1e10]]
    assert list(COCO_STAT_NAMES) == U.STAT_NAMES == DetMetrics.coco_stat_names
    m = DetMetrics(names={0: "a"})
    assert m.coco_stats is None and m.coco_eval is None


def test_case_a():
    b = batch_of([[0, 0, 50, 50], [100, 100, 50, 50]],
                 [[0, 0, 50, 50, 0.9], [300, 300, 50, 50, 0.8], [100, 100, 50, 50, 0.7]])
    stats, pstats, ev, pev, _ = both([b], 1)
    v = (51 + 50 * (2 / 3)) / 101
    want = np.array([v, v, v, -1, v, -1, 0.5, 1, 1, -1, 1, -1])
    assert np.abs(stats - want).max() <= TOL and np.abs(pstats - want).max() <= TOL
    assert_same(ev, pev, stats, pstats)


def test_case_b():
    b = batch_of([[0, 0, 10, 10], [5, 0, 10, 10]], [[2.5, 0, 10, 10, 0.9], [0, 0, 10, 10, 0.8]])
    stats, pstats, ev, pev, imgs = both([b], 1)
    taken = imgs[0][0][4]
    assert (taken[0, :2, 0] == 1).all()  # IoU 0.6 with both labels: the first detection takes the second
    for s in (stats, pstats):
        assert abs(s[1] - 1) <= TOL and abs(s[6] - 0.15) <= TOL and abs(s[7] - 0.65) <= TOL
        assert abs(s[0] - 0.47673267326732673) <= 1e-9 and abs(s[2] - 0.25247524752475248) <= 1e-9
    assert_same(ev, pev, stats, pstats)


def test_case_c():
    b = batch_of([[0, 0, 30, 30]], [[0, 0, 34, 34, 0.9]])
    stats, pstats, ev, pev, _ = both([b], 1)
    # the label is small; the matched medium-sized detection counts for it
    want = np.array([0.6, 1, 1, 0.6, -1, -1, 0.6, 0.6, 0.6, 0.6, -1, -1])
    assert np.abs(stats - want).max() <= TOL and np.abs(pstats - want).max() <= TOL
    assert_same(ev, pev, stats, pstats)


def test_tie_off_threshold():
    """A duplicated label met at IoU 2/3 by one detection: the later label is taken, at every threshold below 2/3,
    and a second identical detection then takes the first."""
    b = batch_of([[0, 0, 50, 20], [0, 0, 50, 20]], [[10, 0, 50, 20, 0.9], [10, 0, 50, 20, 0.8]])
    stats, pstats, ev, pev, imgs = both([b], 1)
    taken, dtm = imgs[0][0][4], imgs[0][0][1]
    assert (taken[0, :4, 0] == 1).all() and (taken[0, :4, 1] == 0).all() and (taken[0, 4:] == -1).all()
    assert dtm[0, :4].all() and not dtm[0, 4:].any()
    assert_same(ev, pev, stats, pstats)
    assert abs(pstats[1] - 1) <= TOL and abs(pstats[0] - 0.4) <= TOL


def test_max_dets_truncation():
    """120 detections of one class on 110 labels: the cut keeps the 100 best, AR1 <= AR10 <= AR100 < 1."""
    labels = [[12 * i, 0, 10, 10] for i in range(110)]
    dets = [[12 * i, 0, 10, 10, 0.99 - 0.005 * ((7 * i) % 120)] for i in range(110)] + \
           [[12 * i, 50, 10, 10, 0.5] for i in range(10)]
    b = batch_of(labels, dets)
    arrays, _ = U.evaluate_batch(*b, 1)
    rank = arrays["rank"][0]
    assert (rank >= 0).sum() == 100 and sorted(rank[rank >= 0]) == list(range(100))
    assert (arrays["matched"][0][rank < 0] == 0).all() and (arrays["ignored"][0][rank < 0] == 0).all()
    stats, pstats, ev, pev, _ = both([b], 1)
    assert_same(ev, pev, stats, pstats)
    assert pstats[6] <= pstats[7] <= pstats[8] < 1 and abs(pstats[6] - 1 / 110) <= TOL
    assert abs(pstats[7] - 10 / 110) <= TOL


def test_empty_category_rules():
    """nc = 4: class 0 labels and detections, class 1 labels only (recall 0, precision 0), class 2 detections only
    and class 3 nothing (both stay -1)."""
    b = batch_of([[0, 0, 40, 40], [100, 0, 40, 40]], [[0, 0, 40, 40, 0.9, 0], [200, 200, 40, 40, 0.8, 2]],
                 classes=[0, 1])
    stats, pstats, ev, pev, _ = both([b], 4)
    assert_same(ev, pev, stats, pstats)
    p, r = pev["precision"], pev["recall"]
    assert (np.abs(p[:, :, 0, 0, 2] - 1) <= TOL).all() and (r[:, 0, 0, 2] == 1).all()
    assert (p[:, :, 1, 0, :] == 0).all() and (r[:, 1, 0, :] == 0).all() and (pev["scores"][:, :, 1, 0, :] == 0).all()
    assert (p[:, :, 2:] == -1).all() and (r[:, 2:] == -1).all()
    assert (p[:, :, :, 1] == -1).all() and (p[:, :, :, 3] == -1).all()  # no small or large label anywhere
    assert abs(pstats[0] - 0.5) <= TOL and pstats[3] == -1 and pstats[5] == -1 and pstats[9] == -1
    # no labels at all: every stat is -1
    e = batch_of([], [[0, 0, 40, 40, 0.9, 0]], classes=[])
    stats, pstats, ev, pev, _ = both([e], 4)
    assert (pstats == -1).all() and (stats == -1).all()


@pytest.mark.parametrize("name", list(U.SCENES))
def test_accumulate_matches_restatement(name):
    batches, nc, single, arrays, imgs, ev, stats = U.reference(name)
    recs = [U.product_record(b[0], a, b[3], b[4], nc, single) for b, a in zip(batches, arrays)]
    pev = coco_accumulate(recs, nc)
    assert pev["counts"] == [10, 101, nc, 4, 3]
    assert_same(ev, pev, stats, coco_summarize(pev))
    lines = coco_summary_lines(pev)
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %0.3f" % stats[0]
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = %0.3f" % stats[1]
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = %0.3f" % stats[6]
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = %0.3f" % stats[11]


@pytest.mark.parametrize("name", list(U.SCENES))
def test_scenes_are_not_trivial(name):
    """The ground the GPU tests stand on: every branch of the protocol is taken in each scene."""
    batches, nc, single, arrays, imgs, ev, stats = U.reference(name)
    c = U.census(imgs)
    print(name, c)
    assert len(c["areas_with_labels"] - {0}) >= 3
    assert c["matched"] > 0 and c["unmatched"] > 0 and c["ig_matched"] > 0 and c["ig_unmatched"] > 0
    assert c["score_ties"] >= 1 and c["iou_ties"] >= 1
    n, max_det, _, _, kws = U.SCENES[name]
    for (det, cnt, boxes, cls, bidx), a in zip(batches, arrays):
        assert det.shape == (n, max_det, 6) and (cnt <= max_det).all()
        assert not single and a["invalid"].sum() > 0 or single and a["invalid"].sum() == 0
        assert (np.diff(bidx) < 0).any() or len(set(bidx.tolist())) == 1  # labels interleaved across images
    if max_det > 100:  # with max_det = 64 no category list reaches the cut
        assert c["cut"] > 0
    if any("many_labels" in kw for kw in kws):
        assert max(np.bincount(b[3].astype(int)).max() for b in batches) > 64
    if any("empty_imgs" in kw for kw in kws):
        assert any((b[1] == 0).any() for b in batches)
        assert any(len(set(range(n)) - set(b[4].tolist())) > 0 for b in batches)


def _desc(**kw):
    thr = np.ascontiguousarray(COCO_IOU_THRS)
    rng = np.ascontiguousarray(COCO_AREA_RNG, dtype=np.float64)
    fake = 256  # a non-null device address: validation never reads it
    d = _lib.CocoDesc(det=fake, det_count=fake, n=2, max_det=300, gt_box=fake, gt_cls=fake, gt_ofs=fake, n_gt=10,
                      single_cls=0, nc=3, iou_thrs=thr.ctypes.data, n_iou=10, area_rng=rng.ctypes.data, n_area=4,
                      max_dets=100, dt_rank=fake, dt_matched=fake, dt_ignored=fake, gt_ignore=fake, invalid=fake,
                      workspace=None)
    for k, v in kw.items():
        setattr(d, k, v)
    d._keep = (thr, rng)
    return d


def test_abi_validation_without_a_launch():
    lib = _lib.lib
    assert lib.ydbl_coco_match(None, None) == 1
    assert "null descriptor" in lib.ydbl_last_error().decode()
    assert lib.ydbl_coco_match(_lib.CocoDesc(), None) == 1
    assert "null buffer" in lib.ydbl_last_error().decode()
    bad = [{"det": None}, {"dt_rank": None}, {"invalid": None}, {"iou_thrs": None}, {"area_rng": None}, {"n": 0},
           {"max_det": 0}, {"n": 65536}, {"max_det": (1 << 20) + 1}, {"n_gt": -1}, {"gt_box": None}, {"gt_ignore": None},
           {"nc": 0}, {"nc": 32768}, {"n_iou": 0}, {"n_iou": 17}, {"n_area": 0}, {"n_area": 9}, {"max_dets": 0},
           {"max_dets": 1025}]
    for kw in bad:
        assert lib.ydbl_coco_match(_desc(**kw), None) == 1, kw
    nan = np.array([0.5, np.nan])
    assert lib.ydbl_coco_match(_desc(iou_thrs=nan.ctypes.data, n_iou=2), None) == 1
    rev = np.array([[10.0, 1.0]])
    assert lib.ydbl_coco_match(_desc(area_rng=rev.ctypes.data, n_area=1), None) == 1
    # capacity: 36 B per detection + 48 B per label must fit 160 KiB, refused before any launch
    assert lib.ydbl_coco_match(_desc(n_gt=3400), None) == 3
    assert "LDS" in lib.ydbl_last_error().decode()
    with pytest.raises(_lib.YdblError):
        _lib.check(lib.ydbl_coco_match(_desc(n_gt=100000), None), "ydbl_coco_match")
    assert lib.ydbl_coco_workspace(2, 300, 10, 3) == 0 and lib.ydbl_coco_workspace(-1, 300, 10, 3) == -1


def test_descriptor_layout_matches_c(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ydbl_coco_desc));']
    for fname, _ in _lib.CocoDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(ydbl_coco_desc, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", str(src), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.splitlines() if line.strip())
    assert int(got["size"]) == C.sizeof(_lib.CocoDesc)
    for fname, _ in _lib.CocoDesc._fields_:
        assert int(got[fname]) == getattr(_lib.CocoDesc, fname).offset, fname
    assert "ydbl_coco_match" in _lib.SIGNATURES and "ydbl_coco_workspace" in _lib.SIGNATURES


def test_val_signature_and_default():
    from ydbl.engine import validator
    from ydbl.engine.model import Model

    p = inspect.signature(Model.val).parameters["coco_eval"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(validator.coco_batch) and hasattr(validator.DetectionValidator, "coco_summary")
    sig = inspect.signature(validator.coco_batch).parameters
    assert list(sig)[:5] == ["det", "count", "gt_box", "gt_cls", "batch_idx"] and "grouped" in sig
