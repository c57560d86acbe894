"""Mask mAP, the host side: the ABI of ydbl_gt_mask_bits / ydbl_mask_iou / ydbl_match_iou and YDBL_MASK_BITS
(struct layouts against gcc, argument validation without a GPU), SegmentMetrics, the dataset's polygon rasteriser
against a brute-force integer point-in-closed-polygon test, and Model.val's guards."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import segval_util as SV

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ydbl.h"
STRUCTS = {"ydbl_gt_bits_desc": "GtBitsDesc", "ydbl_mask_iou_desc": "MaskIouDesc",
           "ydbl_match_iou_desc": "MatchIouDesc", "ydbl_mask_desc": "MaskDesc"}


def test_struct_layout_matches_c(tmp_path):
    from ydbl import _lib

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} %zu\\n", sizeof({cname}));')
        for fname, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'printf("{pyname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("BITS %d\\n", (int)YDBL_MASK_BITS);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.split() for line in out if line.strip())
    assert int(got["BITS"]) == _lib.MASK_BITS == 2
    for cname, pyname in STRUCTS.items():
        st = getattr(_lib, pyname)
        assert int(got[pyname]) == C.sizeof(st), pyname
        for fname, _ in st._fields_:
            assert int(got[f"{pyname}.{fname}"]) == getattr(st, fname).offset, f"{pyname}.{fname}"


def _err():
    from ydbl import _lib

    return _lib.lib.ydbl_last_error().decode()


def test_validation_errors_without_gpu():
    """Every path returns YDBL_EINVAL (1) before anything is launched; the pointers are never dereferenced."""
    from ydbl import _lib

    lib, P = _lib.lib, 4096  # an aligned non-NULL address
    assert lib.ydbl_gt_mask_bits(None, None) == 1 and "null descriptor" in _err()
    assert lib.ydbl_gt_mask_bits(_lib.GtBitsDesc(n=1, n_gt=1), None) == 1 and "null buffer" in _err()
    g = _lib.GtBitsDesc(None, 1, 8, 8, 1, P, 1, 32, 32, P, P)
    assert lib.ydbl_gt_mask_bits(g, None) == 1 and "null buffer" in _err()
    g = _lib.GtBitsDesc(P, 1, 8, 8, 1, P, 1, 32, 32, P + 4, P)
    assert lib.ydbl_gt_mask_bits(g, None) == 1 and "8-byte" in _err()
    g = _lib.GtBitsDesc(P, 1, 8, 8, 1, P, 1, 4097, 4096, P, P)
    assert lib.ydbl_gt_mask_bits(g, None) == 1 and "2^24" in _err()

    assert lib.ydbl_mask_iou(None, None) == 1 and "null descriptor" in _err()
    assert lib.ydbl_mask_iou(_lib.MaskIouDesc(), None) == 1 and "null buffer" in _err()
    full = dict(det_bits=P, row_offset=P, count=P, n=1, max_det=4, gt_bits=P, gt_ofs=P, area_gt=P, n_gt=2,
                out_h=64, out_w=64, iou=P)
    for k in ("det_bits", "row_offset", "count", "gt_ofs", "iou", "gt_bits", "area_gt"):
        assert lib.ydbl_mask_iou(_lib.MaskIouDesc(**{**full, k: None}), None) == 1 and "null buffer" in _err(), k
    assert lib.ydbl_mask_iou(_lib.MaskIouDesc(**{**full, "out_h": 4097, "out_w": 4096}), None) == 1
    assert "2^24" in _err()
    assert lib.ydbl_mask_iou(_lib.MaskIouDesc(**{**full, "det_bits": P + 4}), None) == 1 and "8-byte" in _err()

    assert lib.ydbl_match_iou(None, None) == 1 and "null descriptor" in _err()
    assert lib.ydbl_match_iou(_lib.MatchIouDesc(), None) == 1 and "null buffer" in _err()
    m = _lib.MatchIouDesc(P, P, 1, 4, None, P, P, 2, P, 10, 0, P, P)
    assert lib.ydbl_match_iou(m, None) == 1 and "missing" in _err()
    m = _lib.MatchIouDesc(P, P, 1, 4, P, P, P, 2, P, 33, 0, P, P)
    assert lib.ydbl_match_iou(m, None) == 1 and "n_iou" in _err()

    d = _lib.MaskDesc()
    d.proto = _lib.View(P, 1, 8, 8, 32, 32, _lib.F32)
    d.det, d.count, d.row_offset, d.coef, d.max_det = P, P, P, P, 4
    d.out_h, d.out_w, d.bottom, d.right, d.sx, d.sy = 32, 32, 8, 8, 0.25, 0.25
    d.out, d.out_dtype = P, 3
    assert lib.ydbl_process_mask(d, None) == 1 and "out_dtype" in _err()
    d.out, d.out_dtype = P + 4, _lib.MASK_BITS
    assert lib.ydbl_process_mask(d, None) == 1 and "8-byte" in _err()


def test_pack_mask_bits_matches_the_layout():
    from ydbl.utils.ops import pack_mask_bits

    g = torch.Generator().manual_seed(0)
    for w in (1, 63, 64, 65, 127, 150, 640):
        m = (torch.rand(3, 5, w, generator=g) > 0.5).to(torch.uint8)
        m[0, 0, w - 1] = 1  # the last column, bit 63 of a word where w is a multiple of 64
        assert np.array_equal(SV.words_np(pack_mask_bits(m)), SV.pack_bits(m.numpy())), w


def test_mask_iou_cpu_is_the_reference_expression():
    from ydbl.utils.metrics import mask_iou

    g = torch.Generator().manual_seed(1)
    a, b = (torch.rand(4, 300, generator=g) > 0.5).float(), (torch.rand(6, 300, generator=g) > 0.3).float()
    assert torch.equal(mask_iou(a, b), SV.mask_iou_ref(a, b))


def _stats(seed=0, n=60, nc=3):
    rng = np.random.default_rng(seed)
    tp = np.sort(rng.random((n, 10)) > 0.4, axis=1)[:, ::-1].copy()  # a TP at a threshold is one at every lower
    tp_m = np.sort(rng.random((n, 10)) > 0.55, axis=1)[:, ::-1].copy()
    return tp, tp_m, rng.random(n), rng.integers(0, nc, n).astype(float), rng.integers(0, nc, 40).astype(float)


def test_segment_metrics():
    from ydbl.utils.metrics import DetMetrics, SegmentMetrics, ap_per_class

    tp, tp_m, conf, pc, tc = _stats()
    names = {0: "a", 1: "b", 2: "c"}
    sm, dm, mm = SegmentMetrics(names=names), DetMetrics(names=names), DetMetrics(names=names)
    sm.process(tp, tp_m, conf, pc, tc)
    dm.process(tp, conf, pc, tc)
    mm.process(tp_m, conf, pc, tc)
    assert sm.keys == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP75(B)",
                       "metrics/mAP50-95(B)", "metrics/precision(M)", "metrics/recall(M)", "metrics/mAP50(M)",
                       "metrics/mAP75(M)", "metrics/mAP50-95(M)"]
    assert len(sm.curves) == 8 and len(sm.curves_results) == 8
    assert sm.mean_results() == dm.mean_results() + mm.mean_results() and len(sm.mean_results()) == 10
    for a in ("p", "r", "f1", "all_ap", "ap_class_index"):  # box equals what DetMetrics gives for the same tp
        assert np.array_equal(getattr(sm.box, a), getattr(dm.box, a)), a
        assert np.array_equal(getattr(sm.seg, a), getattr(mm.box, a)), a
    ap = ap_per_class(tp_m, conf, pc, tc)[5]
    assert sm.seg.map50 == float(ap[:, 0].mean()) and sm.seg.map75 == float(ap[:, 5].mean())
    assert sm.seg.map == float(ap.mean()) and sm.seg.map != sm.box.map
    assert sm.class_result(1) == dm.class_result(1) + mm.class_result(1)
    assert np.array_equal(sm.maps, dm.maps + mm.maps)
    assert list(sm.ap_class_index) == list(dm.ap_class_index)
    rd = sm.results_dict
    assert list(rd) == sm.keys + ["fitness"]
    assert [rd[k] for k in sm.keys] == sm.mean_results()
    assert rd["fitness"] == sm.fitness == mm.results_dict["fitness"] + dm.results_dict["fitness"]
    sm.val_loss = [1.0, 2.0, 3.0]
    assert sm.results_dict["val/cls_loss"] == 2.0
    assert sm.confusion_matrix is None and sm.coco_stats is None and sm.task == "segment"


TRIANGLE = [(5.2, 3.9), (58.7, 20.1), (17.0, 50.5)]
CONCAVE = [(10, 10), (80, 12), (80, 60), (45, 30), (12, 58)]
SEGMENT2 = [(7.5, 40.2), (70.9, 11.0)]
OUTSIDE = [(-20.0, -5.0), (50.0, 30.0), (200.0, 20.0), (60.0, 120.0)]
HWS = [(64, 96), (96, 160)]


@pytest.mark.parametrize("hw", HWS, ids=["64x96", "96x160"])
@pytest.mark.parametrize("poly", [TRIANGLE, CONCAVE, SEGMENT2, OUTSIDE, []],
                         ids=["triangle", "concave", "two_points", "outside", "empty"])
def test_polygon_mask_against_brute_force(poly, hw):
    from ydbl.engine.dataset import downsample_mask, polygon_mask

    got = polygon_mask(hw, np.array(poly, dtype=np.float32).reshape(-1, 2))
    want = SV.polygon_mask_ref(hw, poly)
    assert got.dtype == np.uint8 and got.shape == hw
    assert np.array_equal(got, want)
    if poly and poly is not OUTSIDE:
        assert want.sum() > 0
        for px, py in poly:  # a vertex (truncated) lies in the closed polygon
            assert got[int(py), int(px)] == 1
    small = downsample_mask(got)
    assert small.shape == (hw[0] // 4, hw[1] // 4) and np.array_equal(small, SV.downsample_ref(want))


def test_overlap_map_order():
    from ydbl.engine.dataset import polygons2masks_overlap

    hw = (64, 96)
    sq = lambda x0, y0, x1, y1: np.array([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], dtype=np.float32)  # noqa: E731
    # areas on the 1/4 map: big, small (inside big), two of equal area (stable: in label order), an empty one
    polys = [sq(40, 8, 60, 28), sq(4, 4, 90, 60), sq(8, 8, 20, 20), sq(72, 40, 92, 60), np.zeros((0, 2), np.float32),
             sq(40, 40, 60, 60)]
    m, order = polygons2masks_overlap(hw, polys)
    assert m.dtype == np.uint8 and m.shape == (16, 24)
    assert order.tolist() == [1, 0, 3, 5, 2, 4]
    assert m[4, 12] == 2 and m[3, 3] == 5 and m[12, 20] == 3 and m[12, 12] == 4 and m[8, 8] == 1 and m[0, 0] == 0
    assert 6 not in m  # the empty polygon names no pixel
    with pytest.raises(ValueError, match="255"):
        polygons2masks_overlap(hw, [polys[0]] * 256)


@pytest.fixture(scope="module")
def seg_dataset(tmp_path_factory):
    """Three images with polygon rows (one file mixes a box row in, one has box rows only, one is empty)."""
    import dataset_util as D

    root = tmp_path_factory.mktemp("segds")
    D.make_dataset(root, shapes=[(96, 128), (128, 128), (128, 96), (100, 120)], nc=3, labels={}, edge_cases=False)
    lb = root / "labels" / "val"
    (lb / "im000.txt").write_text("0 0.1 0.1 0.5 0.15 0.45 0.6 0.12 0.5\n"
                                  "1 0.2 0.2 0.9 0.2 0.9 0.9 0.2 0.9\n"
                                  "2 0.5 0.5 0.2 0.2\n")
    (lb / "im001.txt").write_text("1 0.5 0.5 0.3 0.3\n0 0.3 0.3 0.2 0.2\n")
    (lb / "im002.txt").write_text("2 0.3 0.3 0.7 0.3 0.7 0.7 0.5 0.5 0.3 0.7\n")
    (lb / "im003.txt").write_text("")
    return root


def test_dataset_masks(seg_dataset):
    from ydbl.engine.dataset import YOLOValDataset, polygons2masks_overlap, split_has_segments

    src = seg_dataset / "images" / "val"
    assert split_has_segments(src)
    plain = YOLOValDataset(src, imgsz=128, batch_size=2, stride=32, num_cls=3)
    seg = YOLOValDataset(src, imgsz=128, batch_size=2, stride=32, num_cls=3, masks=True)
    assert all("segments" not in lb for lb in plain.labels) and all("segments" in lb for lb in seg.labels)
    keys = {"frames", "meta", "shape", "ori_shape", "ratio_pad", "im_file", "cls", "bboxes", "batch_idx"}
    seen = 0
    for pb, sb in zip(plain.batches(), seg.batches()):
        assert set(pb) == keys and set(sb) == keys | {"masks"}  # masks=False: the batch of before, nothing added
        H, W = sb["shape"]
        assert sb["masks"].dtype == np.uint8 and sb["masks"].shape == (len(sb["frames"]), H // 4, W // 4)
        assert pb["im_file"] == sb["im_file"] and np.array_equal(pb["batch_idx"], sb["batch_idx"])
        for j, f in enumerate(sb["im_file"]):
            i = seg.im_files.index(f)
            lbl = seg.labels[i]
            sel = sb["batch_idx"] == j
            (h, w), (top, left) = tuple(sb["meta"][j][2:4]), tuple(sb["meta"][j][4:6])
            polys = [sg * np.float32([w, h]) + np.float32([left, top]) for sg in lbl["segments"]]
            m, order = polygons2masks_overlap((H, W), polys)
            assert np.array_equal(sb["masks"][j], m)
            # cls / bboxes reordered as the map numbers them; masks=False keeps the file's order
            assert np.array_equal(sb["cls"][sel], pb["cls"][sel][order])
            assert np.array_equal(sb["bboxes"][sel], pb["bboxes"][sel][order])
            assert np.array_equal(pb["cls"][sel], plain.labels[i]["cls"].reshape(-1))
            if Path(f).stem == "im001":  # box rows only: labels with empty masks
                assert sel.sum() == 2 and m.max() == 0
            if Path(f).stem == "im000":  # the box row read as a two-point polygon; the big square first
                assert sel.sum() == 3 and sb["cls"][sel][0] == 1 and set(np.unique(m)) >= {1, 2}
            seen += 1
    assert seen == 4


def test_verify_image_label_keeps_its_return(seg_dataset):
    from ydbl.engine.dataset import verify_image_label, verify_image_segments

    im, lb = seg_dataset / "images" / "val" / "im000.png", seg_dataset / "labels" / "val" / "im000.txt"
    out = verify_image_label(str(im), str(lb), 3)
    assert len(out) == 3 and out[1].shape == (3, 5)
    shape, lbs, segs, msg = verify_image_segments(str(im), str(lb), 3)
    assert shape == out[0] and np.array_equal(lbs, out[1]) and len(segs) == 3 and msg == out[2]
    assert [len(s) for s in segs] == [4, 4, 2]


def test_val_guards_on_the_host():
    import seg_util as S
    from ydbl import YOLO

    p = YOLO(str(S.GOLDEN / "yolo11n-seg.json"), nc=3)
    x = torch.zeros(1, 3, 64, 64)
    lab = {"img": x, "bboxes": torch.zeros(0, 4), "cls": torch.zeros(0), "batch_idx": torch.zeros(0)}
    with_m = {**lab, "masks": torch.zeros(1, 16, 16, dtype=torch.uint8)}
    with pytest.raises(ValueError, match="only some batches"):
        p.val([with_m, lab])
    with pytest.raises(ValueError, match="only some batches"):
        p.val([lab, with_m])
    with pytest.raises((ValueError, NotImplementedError), match="gather_rows"):
        p.val([with_m], gather_rows=4)
