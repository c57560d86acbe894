"""The pose models (yolo11-pose.yaml / yolov8-pose.yaml: Pose in place of Detect) on the host: construction from
tests/golden/yolo11-pose.json / yolov8-pose.json, the keypoint branch's width, reference parameter names, the kpt_shape
override and the task; scale_coords / clip_coords, the Keypoints container, PoseMetrics and OKS_SIGMA against the
restatements of tests/pose_util.py; the dataset's pose label rows; the guards raised before a device is touched and the
two new descriptors' layouts.  No GPU."""

import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import pose_util as P

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "ydbl.h"
FAMS = ["yolo11", "yolov8"]


@pytest.mark.parametrize("family", FAMS)
def test_parse_model_and_task(family, golden_dir):
    from ydbl import YOLO
    from ydbl.nn import modules as M

    ref = json.loads((golden_dir / f"{family}.json").read_text())
    pose = json.loads((golden_dir / f"{family}-pose.json").read_text())
    assert pose["backbone"] == ref["backbone"] and pose["head"][:-1] == ref["head"][:-1]
    assert pose["scales"] == ref["scales"] and pose["kpt_shape"] == [17, 3]
    assert pose["head"][-1] == [ref["head"][-1][0], 1, "Pose", ["nc", "kpt_shape"]]
    for scale in "nm":
        p = YOLO(str(golden_dir / f"{family}{scale}-pose.json"), nc=1)
        assert p.task == "pose" and p.model.kpt_shape == [17, 3] and p.model.pose
        head = p.model.model[-1]
        assert type(head) is M.Pose and isinstance(head, M.Detect)
        assert (head.nk, head.nc, tuple(head.kpt_shape)) == (51, 1, (17, 3))
        ch0 = head.cv2[0][0].conv.in_channels
        c4 = max(ch0 // 4, 51)  # head.py:361
        # 51 at scale n of both families; at scale m 64 for yolo11 (256 // 4) and still 51 for yolov8 (192 // 4 = 48)
        assert c4 == {("yolo11", "n"): 51, ("yolo11", "m"): 64, ("yolov8", "n"): 51, ("yolov8", "m"): 51}[family, scale]
        assert all(seq[0].conv.out_channels == c4 and seq[1].conv.out_channels == c4 and seq[2].in_channels == c4
                   and seq[2].out_channels == 51 for seq in head.cv4)
        assert head.legacy is P.FAMILIES[family]
        assert p.model.stride.tolist() == [8.0, 16.0, 32.0]
        o = P.build_oracle(family, scale, 1)
        assert list(p.model.state_dict()) == list(o.state_dict())
        p.model.load_state_dict(o.state_dict(), strict=True)
    p = YOLO(str(golden_dir / f"{family}n-pose.json"), nc=1)
    cm = p.model.compile(2, 64, 64, torch.float16, device="meta")  # shape-only plan
    assert [lv.shape for lv in cm.levels] == [(2, 8, 8, 65), (2, 4, 4, 65), (2, 2, 2, 65)]  # Detect's layout, untouched
    assert [(v.shape, v.cs) for v in cm.plan.pose] == [((2, 8, 8, 51), 56), ((2, 4, 4, 51), 56), ((2, 2, 2, 51), 56)]
    padded = [st for st in cm.plan.steps if st.what == "Conv3x3.pad56"]
    assert len(padded) == 6 and all(st.args[0].y.c == 56 for st in padded)  # the two 3x3 intermediates, zero-padded


def test_kpt_shape_override(golden_dir):
    from ydbl import YOLO

    p = YOLO(str(golden_dir / "yolo11n-pose.json"), nc=2, kpt_shape=[5, 2])
    head = p.model.model[-1]
    assert p.model.kpt_shape == [5, 2] and head.nk == 10 and head.nc == 2 and p.task == "pose"
    assert head.cv4[0][0].conv.out_channels == 16 and head.cv4[0][2].out_channels == 10  # max(64 // 4, 10)
    o = P.build_oracle("yolo11", "n", 2, (5, 2))
    p.model.load_state_dict(o.state_dict(), strict=True)
    assert YOLO(str(golden_dir / "yolo11n.json"), nc=2, kpt_shape=[5, 2]).task == "detect"  # means nothing to Detect


@pytest.mark.parametrize("img0,ratio_pad", [((75, 100), None), ((100, 75), None), ((128, 128), None), ((201, 97), None),
                                            ((75, 100), ((1.25, 1.25), (2.5, 17.0)))])
def test_scale_and_clip_coords(img0, ratio_pad):
    from ydbl.utils import ops

    g = torch.Generator().manual_seed(5)
    pts = torch.rand(6, 17, 3, generator=g) * 160 - 16  # some outside the image on either side
    a = ops.scale_coords((128, 128), pts.clone(), img0, ratio_pad=ratio_pad)
    b = P.scale_coords((128, 128), pts.clone(), img0, ratio_pad=ratio_pad)
    assert torch.equal(a, b) and torch.equal(a[..., 2], pts[..., 2])
    if img0 == (75, 100):  # the issue's 100 x 75 image in 128 x 128: x, y clipped to the image, the third column kept
        assert a[..., 0].max() == 100 and a[..., 1].max() == 75 and a[..., :2].min() == 0
    n = ops.scale_coords((128, 128), pts.clone(), img0, ratio_pad=ratio_pad, normalize=True, padding=False)
    assert torch.equal(n, P.scale_coords((128, 128), pts.clone(), img0, ratio_pad=ratio_pad, normalize=True,
                                         padding=False))
    arr = pts.numpy().copy()
    assert np.array_equal(ops.clip_coords(arr.copy(), (50, 60)), P.clip_coords(arr.copy(), (50, 60)))
    assert torch.equal(ops.clip_coords(pts.clone(), (50, 60)), P.clip_coords(pts.clone(), (50, 60)))
    # unlike scale_boxes the pad is not rounded: 97 wide in 128 at gain 128 / 201 leaves a fractional pad
    if img0 == (201, 97):
        gain = 128 / 201
        padx = (128 - 97 * gain) / 2
        assert padx != round(padx)
        one = ops.scale_coords((128, 128), torch.tensor([[[padx + 10 * gain, 64.0, 1.0]]]), img0)
        assert abs(one[0, 0, 0].item() - 10.0) < 1e-4


def test_keypoints_container():
    from ydbl.engine.results import Keypoints, Results

    data = torch.tensor([[[10.0, 20.0, 0.9], [30.0, 40.0, 0.49], [50.0, 60.0, 0.5]],
                         [[1.0, 2.0, 0.1], [3.0, 4.0, 0.7], [5.0, 6.0, 1.0]]])
    k = Keypoints(data.clone(), (100, 200))
    assert k.has_visible and len(k) == 2 and k.shape == (2, 3, 3)
    want = data.clone()
    want[0, 1, :2] = 0  # visibility < 0.5: xy = 0 (results.py:1305-1311)
    want[1, 0, :2] = 0
    assert torch.equal(k.data, want) and torch.equal(k.xy, want[..., :2]) and torch.equal(k.conf, want[..., 2])
    assert torch.equal(k.xyn, want[..., :2] / torch.tensor([200.0, 100.0]))
    assert len(k[1:]) == 1 and torch.equal(k[1].data, want[1:2])  # a 2-D row becomes [1, K, 3]
    assert isinstance(k.numpy().data, np.ndarray) and k.cpu().data.device.type == "cpu"
    two = Keypoints(data[..., :2].clone(), (100, 200))
    assert not two.has_visible and two.conf is None and torch.equal(two.xy, data[..., :2])
    empty = Keypoints(torch.zeros(0, 17, 3), (64, 64))
    assert len(empty) == 0 and empty.xy.shape == (0, 17, 2) and empty.xyn.shape == (0, 17, 2)
    boxes = torch.tensor([[1.0, 2.0, 30.0, 40.0, 0.9, 0.0], [5.0, 6.0, 70.0, 80.0, 0.8, 0.0]])
    r = Results(None, "a.jpg", {0: "person"}, boxes=boxes, orig_shape=(100, 200), keypoints=data.clone())
    assert r.keypoints is not None and len(r[0].keypoints) == 1 and r.masks is None
    s = r.summary()
    assert s[0]["keypoints"]["x"] == [10.0, 0.0, 50.0] and s[1]["keypoints"]["visible"] == pytest.approx([0.1, 0.7, 1.0])
    assert r.summary(normalize=True)[0]["keypoints"]["x"] == pytest.approx([0.05, 0.0, 0.25])  # (fp32 values)
    with pytest.raises(NotImplementedError, match="keypoints"):
        r.plot()
    none = Results(None, "a.jpg", {0: "person"}, boxes=boxes, orig_shape=(100, 200))
    assert none.keypoints is None


def test_results_save_txt_carries_keypoints(tmp_path):
    from ydbl.engine.results import Results

    boxes = torch.tensor([[10.0, 20.0, 30.0, 40.0, 0.9, 0.0]])
    kp = torch.tensor([[[20.0, 10.0, 0.75], [100.0, 50.0, 0.25]]])
    r = Results(None, "a.jpg", {0: "person"}, boxes=boxes, orig_shape=(100, 200), keypoints=kp)
    r.save_txt(tmp_path / "a.txt", save_conf=True)
    row = [float(v) for v in (tmp_path / "a.txt").read_text().split()]
    # cls, xywhn, then x y v per keypoint (the invisible one zeroed), then conf (results.py:705-713)
    assert row == pytest.approx([0, 0.1, 0.3, 0.1, 0.2, 0.1, 0.1, 0.75, 0.0, 0.0, 0.25, 0.9])


def test_pose_metrics_and_sigma():
    from ydbl.utils.metrics import OKS_SIGMA, PoseMetrics, kpt_iou, metric_fitness

    assert len(OKS_SIGMA) == 17 and float(OKS_SIGMA.sum()) == pytest.approx(float(P.OKS_SIGMA.sum()), abs=0)
    assert np.array_equal(OKS_SIGMA, P.OKS_SIGMA)
    m = PoseMetrics(names={0: "person", 1: "dog"})
    assert m.task == "pose"
    assert m.keys == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP75(B)",
                      "metrics/mAP50-95(B)", "metrics/precision(P)", "metrics/recall(P)", "metrics/mAP50(P)",
                      "metrics/mAP75(P)", "metrics/mAP50-95(P)"]
    rng = np.random.default_rng(0)
    n = 40
    tp, tp_p = rng.random((n, 10)) < 0.6, rng.random((n, 10)) < 0.4
    conf, pc = rng.random(n).astype(np.float32), rng.integers(0, 2, n).astype(np.float32)
    tc = rng.integers(0, 2, 30).astype(np.float32)
    m.process(tp, tp_p, conf, pc, tc)
    assert m.pose.map != m.box.map and len(m.mean_results()) == 10
    assert m.fitness == pytest.approx(metric_fitness(m.pose) + metric_fitness(m.box))
    d = m.results_dict
    assert list(d) == m.keys + ["fitness"] and d["metrics/mAP50(P)"] == m.pose.map50 and d["fitness"] == m.fitness
    g = torch.Generator().manual_seed(1)
    k1, k2 = torch.rand(3, 17, 3, generator=g) * 50, torch.rand(4, 17, 3, generator=g) * 50
    k1[0, :, 2] = 0
    area = torch.tensor([100.0, 0.0, 900.0])
    assert torch.equal(kpt_iou(k1, k2, area, OKS_SIGMA), P.kpt_iou(k1, k2, area, P.OKS_SIGMA))


def test_pose_validator_desc_and_sigma(golden_dir):
    from ydbl import YOLO
    from ydbl.engine.validator import PoseValidator
    from ydbl.utils.metrics import OKS_SIGMA, PoseMetrics

    v = PoseValidator(YOLO(str(golden_dir / "yolo11n-pose.json"), nc=1), {})
    assert v.stat_keys == ("tp", "tp_p", "conf", "pred_cls", "target_cls") and isinstance(v.metrics, PoseMetrics)
    assert np.array_equal(v.sigma, OKS_SIGMA)
    assert "Pose(P" in v.get_desc() and "Box(P" in v.get_desc() and len(v.get_desc().split()) == 13
    v5 = PoseValidator(YOLO(str(golden_dir / "yolo11n-pose.json"), nc=1, kpt_shape=[5, 2]), {})
    assert np.array_equal(v5.sigma, np.ones(5) / 5)


def _pose_row(cls, box, kpts):
    return f"{cls} " + " ".join(f"{v:.6f}" for v in [*box, *np.asarray(kpts).reshape(-1)])


def test_dataset_pose_rows(tmp_path):
    import dataset_util as D
    from ydbl.engine.dataset import YOLOValDataset, split_has_keypoints, verify_image_keypoints

    D.make_dataset(tmp_path, shapes=[(96, 128), (100, 128)], nc=1, labels={}, edge_cases=False)
    lb, im = tmp_path / "labels" / "val", tmp_path / "images" / "val"
    rng = np.random.default_rng(3)
    k0 = np.concatenate([rng.uniform(0.1, 0.9, (2, 17, 2)), rng.integers(0, 3, (2, 17, 1))], -1)
    (lb / "im000.txt").write_text("\n".join(_pose_row(0, b, k) for b, k in zip(
        [[0.5, 0.5, 0.4, 0.6], [0.3, 0.4, 0.2, 0.2]], k0)) + "\n")
    (lb / "im001.txt").write_text("")
    shape, rows, kpts, msg = verify_image_keypoints(str(im / "im000.png"), str(lb / "im000.txt"), 1, (17, 3))
    assert shape == (96, 128) and rows.shape == (2, 5) and kpts.shape == (2, 17, 3) and not msg
    order = np.lexsort(rows.T[::-1])  # (np.unique's row order: the duplicate check sorts nothing here but be exact)
    assert np.allclose(np.sort(kpts.reshape(2, -1), 0), np.sort(k0.reshape(2, -1).astype(np.float32), 0), atol=1e-6)
    assert len(order) == 2 and split_has_keypoints(im, (17, 3)) and not split_has_keypoints(im, (5, 2))
    # ndim == 2 rows get the visibility column (1: the reference rejects negative values before it could be 0)
    k2 = rng.uniform(0.1, 0.9, (1, 5, 2))
    (lb / "im001.txt").write_text(_pose_row(0, [0.5, 0.5, 0.2, 0.2], k2[0]) + "\n")
    _, rows2, kp2, _ = verify_image_keypoints(str(im / "im001.png"), str(lb / "im001.txt"), 1, (5, 2))
    assert rows2.shape == (1, 5) and kp2.shape == (1, 5, 3) and (kp2[..., 2] == 1).all()
    assert np.allclose(kp2[..., :2], k2, atol=1e-6)
    # a wrong column count is rejected (the pair is skipped with a message)
    shape3, _, _, msg3 = verify_image_keypoints(str(im / "im001.png"), str(lb / "im001.txt"), 1, (17, 3))
    assert shape3 is None and "56 columns" in msg3
    (lb / "im001.txt").write_text("")
    ds = YOLOValDataset(im, imgsz=128, batch_size=4, stride=32, num_cls=1, keypoints=True, kpt_shape=(17, 3))
    hb = next(iter(ds.batches()))
    assert hb["keypoints"].shape == (2, 17, 3) and hb["keypoints"].dtype == np.float32 and len(hb["cls"]) == 2
    # the keypoints follow the boxes through the letterbox: back in native pixels they are the file's values
    H, W = hb["shape"]
    kp = torch.from_numpy(hb["keypoints"]).clone()
    kp[..., 0] *= W
    kp[..., 1] *= H
    si = int(hb["batch_idx"][0])
    nat = P.scale_coords((H, W), kp, hb["ori_shape"][si], ratio_pad=hb["ratio_pad"][si])
    got = np.sort(nat.numpy().reshape(2, -1), 0)
    want = k0.copy()
    want[..., 0] *= 128
    want[..., 1] *= 96
    assert np.allclose(got, np.sort(want.reshape(2, -1), 0), atol=1e-3)
    with pytest.raises(ValueError, match="kpt_shape"):
        YOLOValDataset(im, imgsz=128, num_cls=1, keypoints=True)


def test_guards_raise_before_a_device_is_touched(golden_dir):
    """fp8, the loss and the batch-sharded predictor: NotImplementedError from the host checks (there is no GPU here:
    anything that reached for a device would raise something else)."""
    from ydbl import YOLO
    from ydbl.engine.session import DetectSession, check_pose, is_pose
    from ydbl.parallel import ShardedPredictor

    p = YOLO(str(golden_dir / "yolo11n-pose.json"), nc=1)
    assert is_pose(p.model) and not is_pose(YOLO(str(golden_dir / "yolo11n.json"), nc=1).model)
    check_pose(p.model)
    with pytest.raises(NotImplementedError, match="fp8"):
        p.session(1, 64, 64, fp8=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        DetectSession(p.model, 1, 64, 64, torch.float16, fp8=True)
    with pytest.raises(NotImplementedError, match="fp8"):
        p.predict(torch.zeros(1, 3, 64, 64), fp8=True)
    with pytest.raises(NotImplementedError, match="v8PoseLoss"):
        p.session(1, 64, 64, loss=True)
    with pytest.raises(NotImplementedError, match="v8PoseLoss"):
        p.model.loss({"img": torch.zeros(1, 3, 64, 64), "batch_idx": torch.zeros(0), "cls": torch.zeros(0, 1),
                      "bboxes": torch.zeros(0, 4)})
    with pytest.raises(NotImplementedError, match="v8PoseLoss"):
        p.model.init_criterion()
    with pytest.raises(NotImplementedError, match="v8PoseLoss"):
        p.val([], loss=True)
    with pytest.raises(NotImplementedError, match="batch-sharded"):
        ShardedPredictor(p, 4, 64, 64, device=0)


def test_new_descriptors_match_c(tmp_path):
    """The ctypes mirrors of ydbl_pose_kpt_desc and ydbl_kpt_oks_desc against gcc's sizeof / offsetof."""
    from ydbl import _lib

    structs = {"ydbl_pose_kpt_desc": "PoseKptDesc", "ydbl_kpt_oks_desc": "KptOksDesc"}
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


def test_new_entry_points_refuse_bad_descriptors():
    from ydbl import _lib

    lib = _lib.lib
    assert lib.ydbl_pose_keypoints(None, None) == 1 and lib.ydbl_kpt_oks(None, None) == 1
    d = _lib.PoseKptDesc()
    d.keep_idx, d.count, d.out = 16, 16, 16
    d.nl, d.n, d.max_det, d.K, d.ndim = 1, 1, 8, 17, 4
    assert lib.ydbl_pose_keypoints(d, None) == 1 and "ndim" in lib.ydbl_last_error().decode()
    d.ndim = 3
    d.kpt[0] = _lib.View(16, 1, 2, 2, 50, 56, _lib.F16)  # 50 channels are not 17 * 3
    assert lib.ydbl_pose_keypoints(d, None) == 1 and "K * ndim" in lib.ydbl_last_error().decode()
    d.kpt[0] = _lib.View(16, 1, 2, 2, 51, 56, _lib.F16)
    d.max_det = 5000
    assert lib.ydbl_pose_keypoints(d, None) == 1 and "max_det" in lib.ydbl_last_error().decode()
    o = _lib.KptOksDesc()
    o.pred_kpts, o.count, o.gt_ofs, o.sigma = 16, 16, 16, 16
    o.n, o.max_det, o.K, o.ndim = 1, 8, 65, 3
    assert lib.ydbl_kpt_oks(o, None) == 1 and "[1, 64]" in lib.ydbl_last_error().decode()
    o.K, o.n_gt = 17, 2
    assert lib.ydbl_kpt_oks(o, None) == 1 and "labels missing" in lib.ydbl_last_error().decode()
