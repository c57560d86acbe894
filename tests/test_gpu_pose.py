"""The pose models on the MI355X: yolo11n-pose / yolov8n-pose end to end (128^2 and 96 x 160, nc 1, kpt_shape
[17, 3], trained-like BN, batch 2, fp32 and half), built as the segmentation pair is (tests/pose_util.py: restated
oracle, sensitize_, weights copied).

model(x) has the reference's shapes and dtypes; ycat[:, :5] and the raw keypoint map lie within parity_util's fp32_rule /
fp16_rule of the restatement's legs.  predict()'s boxes are the detection twin's (the same weights under a Detect head)
up to the pose predictor's rounding; the session's keypoints EQUAL (x, y) the fp32 decode of its own raw maps at the
anchors keep_idx names, the visibility within the fp32 elementwise bound of the fp64 sigmoid, and
results[i].keypoints.data EQUALS scale_coords of the session's keypoints under the Keypoints rule -- kernel, gather and
scaling end to end.  Then the multi-label index (nc = 2), the letterbox path, track(), val() with and without
keypoints, on tensor batches and on a dataset, and the guards."""

import copy
import math
import warnings

import numpy as np
import pytest
import torch

import pose_util as P

pytestmark = pytest.mark.gpu
FAMILIES = ["yolo11", "yolov8"]
CONF = 0.25
HWS = [(128, 128), (96, 160)]
STRIDES = [8.0, 16.0, 32.0]


def _logit(v):
    return math.log(v / (1 - v))


def images(hw):
    """Image 0 random, image 1 black: their best class scores differ by a wide margin."""
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[1]))
    x[1] = 0.0
    return x


def level_hws(hw):
    return [(hw[0] // int(s), hw[1] // int(s)) for s in STRIDES]


@pytest.fixture(scope="module")
def pairs():
    """family -> (product, fused restatement, detection twin): the class bias of all three shifted by one constant so
    that, on the 128^2 test batch, image 0's k-th best anchor scores above CONF and image 1's best below it (k the
    largest of 6..2 that leaves a gap of 0.2 in logits: 6 for yolo11, 4 for yolov8)."""
    from ydbl import YOLO

    cache = {}

    def get(family):
        if family not in cache:
            x = images((128, 128))
            p, o = P.build_pair(family, "n", 1, x)
            with torch.no_grad():
                z = torch.logit(o(x)[0][:, 4].double())
            top, lo = z[0].topk(6).values.tolist(), z[1].max().item()
            ks = [k for k in range(6, 1, -1) if top[k - 1] - lo > 0.2]  # 0.2: far more than the fp16 noise of a logit
            assert ks, (top, lo)
            hi = top[ks[0] - 1]
            delta = _logit(CONF) - (hi + lo) / 2
            with torch.no_grad():
                for m in (p.model.model[-1], o.model[-1]):
                    for seq in m.cv3:
                        seq[-1].bias += delta
            p.reset_sessions()
            twin = YOLO(str(P.GOLDEN / f"{family}n.json"), nc=1)
            missing, unexpected = twin.model.load_state_dict(p.model.state_dict(), strict=False)
            assert not missing and all(".cv4." in k for k in unexpected)
            cache[family] = (p, o, twin)
        return cache[family]

    return get


@pytest.fixture(scope="module")
def conf_of(pairs):
    """(family, hw) -> the conf threshold of the shape: CONF at 128^2; elsewhere between image 0's 6th and 7th best
    anchor scores of the restatement's fp32 leg, so that image 0 has about six detections."""
    cache = {}

    def get(family, hw):
        if hw == (128, 128):
            return CONF
        if (family, hw) not in cache:
            with torch.no_grad():
                sc = pairs(family)[1](images(hw))[0][0, 4].topk(7).values
            cache[(family, hw)] = float((sc[5] + sc[6]) / 2)
        return cache[(family, hw)]

    return get


def dev_stats(t, t64):
    d = (t.double() - t64).abs().flatten()
    q = torch.quantile(d[torch.randperm(d.numel(), generator=torch.Generator().manual_seed(0))[:1 << 20]], 0.999)
    return {"box_max": d.max().item(), "box_p999": q.item(), "conf_max": 0.0, "conf_p999": 0.0}


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("hw", HWS, ids=["128x128", "96x160"])
@pytest.mark.parametrize("family", FAMILIES)
def test_model_forward(pairs, family, hw, half):
    from parity_util import err_stats, fp16_rule, fp32_rule

    p, o, _ = pairs(family)
    x = images(hw)
    with torch.inference_mode():
        r64 = copy.deepcopy(o).double()(x.double())
        rleg = copy.deepcopy(o).half()(x.half()) if half else o(x)
    ycat, (feats, kpt) = p.model(x.cuda().half() if half else x.cuda())
    torch.cuda.synchronize()
    A = sum(h * w for h, w in level_hws(hw))
    assert ycat.shape == (2, 4 + 1 + 51, A) and kpt.shape == (2, 51, A)
    assert [tuple(f.shape) for f in feats] == [(2, 65, h, w) for h, w in level_hws(hw)]
    assert ycat.dtype == kpt.dtype == feats[0].dtype == (torch.float16 if half else torch.float32)
    rule, key = (fp16_rule, "box_p999") if half else (fp32_rule, "box_max")
    st, st_ref = err_stats(ycat[:, :5].cpu(), r64[0][:, :5]), err_stats(rleg[0][:, :5].float(), r64[0][:, :5])
    tb, tc = rule(st_ref)
    print(f"{family}n-pose {hw} {'half' if half else 'fp32'} y: gpu {st} | leg {st_ref}")
    assert st[key] <= tb and st[key.replace("box", "conf")] <= tc
    sg, sl = dev_stats(kpt.cpu(), r64[1][1]), dev_stats(rleg[1][1].float(), r64[1][1])
    print(f"{family}n-pose {hw} {'half' if half else 'fp32'} kpt: gpu {sg[key]:.3g} leg {sl[key]:.3g} "
          f"bound {rule(sl)[0]:.3g}")
    assert sg[key] <= rule(sl)[0]
    # the decoded part is kpts_decode of the returned raw map, in its dtype (fp32: x / y exactly torch's on the CPU)
    want = P.kpts_decode(kpt.cpu().float(), level_hws(hw), STRIDES, 3)
    got = ycat[:, 5:].cpu().float().reshape(2, 17, 3, A)
    want = want.reshape(2, 17, 3, A)
    if not half:
        assert torch.equal(got[:, :, :2], want[:, :, :2])
    assert torch.allclose(got[:, :, 2], want[:, :, 2], rtol=0, atol=2e-3 if half else 1e-5)


def session_state(p):
    """The most recently used session and its det, counts, kept indices, keypoints and raw maps, on the host."""
    s = list(p._sessions.values())[-1]
    raw = s.pose_outputs()
    keep = torch.cat([part.keep_idx for part in s.parts])
    torch.cuda.synchronize()
    return s, s.det.cpu(), s.count.cpu().tolist(), keep.cpu(), s.kpts.cpu(), raw.float().cpu()


def check_session_keypoints(p, hw, nc=0, counts=None):
    """s.kpts against the fp32 decode of the session's own raw maps at the anchors keep_idx names: x / y equal, the
    visibility within rtol = atol = 1e-5 of the fp64 sigmoid, slots past the count zero.  counts: the images' counts
    when the launch wrote det | count into a binding slot (predict() on a device batch) and not into the session's."""
    s, det, own, keep, kpts, raw = session_state(p)
    counts = own if counts is None else counts
    for i, k in enumerate(counts):
        assert (kpts[i, k:] == 0).all()
        if k == 0:
            continue
        assert (keep[i, :k] >= 0).all()
        anchors = keep[i, :k].long() // nc if nc else keep[i, :k].long()
        rows = raw[i][:, anchors].t().contiguous()
        want = P.decode_rows(rows, anchors, level_hws(hw), STRIDES, 3)
        assert torch.equal(kpts[i, :k, :, :2], want[..., :2]), i
        v64 = rows.double().reshape(k, 17, 3)[..., 2].sigmoid()
        assert torch.allclose(kpts[i, :k, :, 2].double(), v64, rtol=1e-5, atol=1e-5)
    return s, det, counts, keep, kpts


def keypoints_rule(k):
    """Keypoints.__init__ (results.py:1305-1311) on a copy."""
    k = k.clone()
    k[..., :2][k[..., 2] < 0.5] = 0
    return k


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("hw", HWS, ids=["128x128", "96x160"])
@pytest.mark.parametrize("family", FAMILIES)
def test_predict_boxes_and_keypoints(pairs, conf_of, family, hw, half):
    p, _, twin = pairs(family)
    x = images(hw).cuda()
    conf = conf_of(family, hw)
    res = p.predict(x, conf=conf, half=half)  # (a contiguous fp32 device batch: the bound-input path)
    s, det, counts, keep, kpts = check_session_keypoints(p, hw, counts=[len(r.boxes) for r in res])
    assert counts[0] > 0
    det_res = twin.predict(x, conf=conf, half=half)
    for i, (a, b) in enumerate(zip(res, det_res)):
        assert len(a.boxes) == len(b.boxes)
        assert torch.equal(a.boxes.data[:, :4], b.boxes.data[:, :4].round())  # pose/predict.py:50
        assert torch.equal(a.boxes.data[:, 4:], b.boxes.data[:, 4:]) and b.keypoints is None
        want = keypoints_rule(P.scale_coords(hw, kpts[i, :len(a.boxes)].clone(), hw))
        assert a.keypoints.data.shape == (len(a.boxes), 17, 3) and torch.equal(a.keypoints.data.cpu(), want)
    if hw == (128, 128):  # the batch the bias was set on: detections in image 0, none in image 1
        assert counts[1] == 0 and res[1].keypoints is not None and res[1].keypoints.data.shape == (0, 17, 3)
        assert (res[0].keypoints.data[..., 2] >= 0.5).any() or (res[0].keypoints.xy == 0).all()
        # a second call takes the other binding slot; the first call's results keep their values
        first = res[0].keypoints.data.clone()
        again = p.predict(x, conf=conf, half=half)
        assert torch.equal(again[0].keypoints.data, first) and torch.equal(res[0].keypoints.data, first)
        # the copy path (a host batch) and batch 4 (two sub-batch plans, each writing its rows of one kpts buffer)
        host = p.predict(x.cpu(), conf=conf, half=half)
        assert torch.equal(host[0].keypoints.data, first) and torch.equal(host[0].boxes.data, res[0].boxes.data)
        four = p.predict(torch.cat([x, x]), conf=conf, half=half)
        assert len(list(p._sessions.values())[-1].children) == 2
        assert torch.equal(four[0].keypoints.data, first) and torch.equal(four[2].keypoints.data, first)
        assert four[1].keypoints.data.shape == (0, 17, 3) and torch.equal(four[2].boxes.data, res[0].boxes.data)
    one = res[0][:1]
    assert len(one.keypoints) == 1 and res[0].cpu().keypoints.data.device.type == "cpu"
    assert len(res[0].summary()) == counts[0] and len(res[0].summary()[0]["keypoints"]["x"]) == 17


def test_predict_image_files(pairs, tmp_path):
    """Two image files of different shapes in one batch: the letterbox path, boxes and keypoints in each image's own
    pixels."""
    from PIL import Image

    p, _, _ = pairs("yolo11")
    g = torch.Generator().manual_seed(3)
    shapes = [(150, 200), (190, 120)]
    paths = []
    for i, (h, w) in enumerate(shapes):
        a = (torch.rand(h, w, 3, generator=g) * 255).byte().numpy()
        paths.append(str(tmp_path / f"im{i}.png"))
        Image.fromarray(a).save(paths[-1])
    res = p.predict(paths, conf=0.05, half=True, imgsz=128, batch=2)
    s, det, counts, keep, kpts, _ = session_state(p)
    assert sum(counts) > 0
    for i, (r, shp) in enumerate(zip(res, shapes)):
        assert r.orig_shape == shp and len(r.boxes) == counts[i]
        b = r.boxes.data[:, :4]
        assert torch.equal(b, b.round()) and (b[:, [0, 2]] <= shp[1]).all() and (b[:, [1, 3]] <= shp[0]).all()
        # the restated scale_coords evaluated by torch on the device, as the predictor's runs there (torch's CUDA
        # division by a Python scalar multiplies by its reciprocal: the CPU's quotient can differ in the last bit)
        want = keypoints_rule(P.scale_coords((s.h, s.w), kpts[i, :counts[i]].clone().cuda(), shp)).cpu()
        assert torch.equal(r.keypoints.data.cpu(), want)
        cpu = keypoints_rule(P.scale_coords((s.h, s.w), kpts[i, :counts[i]].clone(), shp))
        assert torch.allclose(want, cpu, rtol=1e-6, atol=1e-5)
        assert (r.keypoints.xy[..., 0] <= shp[1]).all() and (r.keypoints.xy[..., 1] <= shp[0]).all()


def test_multi_label_index():
    """nc = 2 at val-style thresholds: keep_idx is anchor * nc + cls and the kernel divides by nc."""
    x = images((128, 128))
    p, _ = P.build_pair("yolo11", "n", 2, x)
    s = p.session(2, 128, 128, half=True, conf=0.001, multi_label=True, max_det=300)
    s(x.cuda())
    assert s.multi_label
    _, det, counts, keep, kpts = check_session_keypoints(p, (128, 128), nc=2)
    assert counts[0] > 8 and (keep[0, :counts[0]] % 2 == 1).any() and (keep[0, :counts[0]] % 2 == 0).any()
    assert torch.equal(keep[0, :counts[0]] % 2, det[0, :counts[0], 5].int())  # the index's class is the row's


def test_track_carries_keypoints(pairs):
    p, _, _ = pairs("yolo11")
    x = images((128, 128)).cuda()
    pred = p.predict(x, conf=CONF, half=True)
    res = p.track(x, conf=CONF, half=True)
    assert len(res[0].boxes) > 0 and len(res[1].boxes) == 0 and res[1].keypoints.data.shape == (0, 17, 3)
    k = res[0].keypoints.data
    assert len(res[0].keypoints) == len(res[0].boxes) and k.shape[1:] == (17, 3)
    pool = pred[0].keypoints.data
    for j in range(len(k)):  # each row's keypoints are those of the detection it was matched to
        assert any(torch.equal(k[j], pool[q]) for q in range(len(pool)))


def same_blocks(got, want):
    return len(got) == len(want) and all(torch.equal(torch.as_tensor(a).bool(), torch.as_tensor(b).bool())
                                         for a, b in zip(got, want))


VAL_IOU = 0.95  # the NMS threshold of the val test: the few anchors above CONF overlap, 0.7 would leave one of them


def labels_from_predictions(p, x, conf, half=True):
    """A tensor batch whose labels shadow image 0's own predictions: label l is detection l's box and its keypoints
    moved by a constant offset, chosen by bisection (fp64 restatement) so that the pair's OKS is TARGETS[l] -- in the
    middle between two thresholds.  Image 1 gets one label nothing predicts."""
    targets = [0.975, 0.825, 0.625, 0.525]
    res = p.predict(x.cuda(), conf=conf, iou=VAL_IOU, half=half)
    n = min(len(res[0].boxes), len(targets))
    assert n >= 2
    s, det, counts, keep, kpts, _ = session_state(p)
    boxes = res[0].boxes.data[:n, :4].cpu().clone()  # (predict() on a device batch writes det into a binding slot)
    gk = P.clip_coords(kpts[0, :n].clone(), x.shape[2:])
    gk[..., 2] = 2.0
    gk[:, 1::2, 2] = 0.0  # every other point invisible
    for l in range(n):
        lo, hi = 0.0, 64.0
        for _ in range(60):
            mid = (lo + hi) / 2
            g = gk[l:l + 1].double().clone()
            g[..., 0] += mid
            v = P.kpt_iou(g, gk[l:l + 1].double(), P.gt_area(boxes[l:l + 1].double()), P.OKS_SIGMA).item()
            lo, hi = (mid, hi) if v > targets[l] else (lo, mid)
        gk[l, :, 0] += lo
    boxes = torch.cat([boxes, torch.tensor([[5.0, 5.0, 40.0, 50.0]])])
    gk = torch.cat([gk, torch.rand(1, 17, 3, generator=torch.Generator().manual_seed(1)) * 40])
    return {"img": x, "bboxes": boxes, "cls": torch.zeros(n + 1), "batch_idx": torch.tensor([0] * n + [1]),
            "keypoints": gk}


def restated_tp_p(p, batch, hw):
    """(tp_p blocks, smallest threshold margin) of the restated validator on the session's own det and keypoints."""
    s, det, counts, keep, kpts, _ = session_state(p)
    pk = P.clip_coords(kpts.clone(), hw)  # scale_coords at gain 1, pad 0
    gk = P.clip_coords(batch["keypoints"].clone(), hw)
    blocks = P.tp_p_ref(det, counts, pk, gk, batch["bboxes"], batch["cls"], batch["batch_idx"], P.OKS_SIGMA)
    ref = P.oks_ref(pk, counts, gk, batch["bboxes"], batch["batch_idx"], P.OKS_SIGMA, torch.float64)
    return blocks, P.threshold_margin(ref, batch["cls"], batch["batch_idx"], det, counts), ref


@pytest.mark.parametrize("family", FAMILIES)
def test_val_with_keypoints(pairs, family):
    from ydbl.utils.metrics import PoseMetrics

    p, _, _ = pairs(family)
    hw = (128, 128)
    x = images(hw)
    batch = labels_from_predictions(p, x, CONF)
    metrics = p.val([batch], half=True, conf=CONF, iou=VAL_IOU)
    assert isinstance(metrics, PoseMetrics)
    v = p.validator
    want, margin, ref = restated_tp_p(p, batch, hw)
    print(f"{family}: OKS margin {margin:.3g}; label-vs-own-detection OKS {ref[0][1].diagonal().tolist()}")
    assert margin >= 1e-4  # the precondition: no same-class pair within 1e-4 of a threshold
    assert same_blocks(v.stats["tp_p"], want)
    tp_p = torch.cat(v.stats["tp_p"])
    assert tp_p[:, 0].sum() >= 2 and not tp_p[:, -1].all()  # some OKS values are high, the thresholds separate them
    assert sum(len(t) for t in v.stats["tp_p"]) == sum(len(t) for t in v.stats["tp"])
    assert metrics.pose.map50 > 0 and metrics.box.map50 > 0
    assert set(metrics.results_dict) == set(PoseMetrics.keys) | {"fitness"}
    # two-column ground truth gets the visibility column (every point visible)
    two = {**batch, "keypoints": batch["keypoints"][..., :2].clone()}
    p.val([two], half=True, conf=CONF, iou=VAL_IOU)
    full = {**batch, "keypoints": torch.cat([two["keypoints"], torch.ones(len(two["keypoints"]), 17, 1)], -1)}
    assert same_blocks(p.validator.stats["tp_p"], restated_tp_p(p, full, hw)[0])
    with pytest.raises(ValueError, match="only some"):
        p.val([batch, {k: v_ for k, v_ in batch.items() if k != "keypoints"}], half=True, conf=CONF)


def test_val_without_keypoints_warns(pairs):
    import ydbl.engine.model as em
    from ydbl.utils.metrics import DetMetrics

    p, _, _ = pairs("yolo11")
    x = images((96, 160))
    boxes = torch.tensor([[10.0, 10.0, 60.0, 50.0], [30.0, 20.0, 120.0, 90.0], [5.0, 40.0, 70.0, 80.0]])
    batch = {"img": x, "bboxes": boxes, "cls": torch.zeros(3), "batch_idx": torch.tensor([0, 0, 1])}
    em._POSE_VAL_WARNED = False
    with pytest.warns(UserWarning, match="keypoint metrics"):
        metrics = p.val([batch], half=True)
    assert isinstance(metrics, DetMetrics) and len(torch.cat(p.validator.stats["target_cls"])) == 3
    assert "tp_p" not in p.validator.stats
    with warnings.catch_warnings():  # said once
        warnings.simplefilter("error")
        em._warn_pose_val()


def test_val_dataset_with_pose_rows(pairs, tmp_path):
    """A three-image dataset whose label rows have 5 + 51 columns: PoseMetrics, and tp_p equal to the restated
    validator fed the session's own detections and keypoints in native space (one batch: the session still holds
    it), save_json rows with "keypoints"."""
    import json

    import dataset_util as D
    from ydbl.engine.dataset import YOLOValDataset
    from ydbl.engine.validator import native_labels
    from ydbl.utils.metrics import PoseMetrics

    p, _, _ = pairs("yolo11")
    D.make_dataset(tmp_path, shapes=[(96, 128), (100, 128), (90, 120)], nc=1, labels={}, edge_cases=False)
    lb = tmp_path / "labels" / "val"
    rng = np.random.default_rng(5)

    def row(box):
        k = np.concatenate([box[0] + (rng.uniform(-0.5, 0.5, (17, 1))) * box[2],
                            box[1] + (rng.uniform(-0.5, 0.5, (17, 1))) * box[3], rng.integers(0, 3, (17, 1))], 1)
        return "0 " + " ".join(f"{v:.6f}" for v in [*box, *k.reshape(-1)])

    (lb / "im000.txt").write_text(row([0.5, 0.5, 0.4, 0.6]) + "\n" + row([0.3, 0.4, 0.2, 0.2]) + "\n")
    (lb / "im001.txt").write_text(row([0.6, 0.5, 0.5, 0.5]) + "\n")
    (lb / "im002.txt").write_text("")
    out = tmp_path / "out"
    metrics = p.val(data=str(tmp_path / "data.yaml"), imgsz=128, batch=4, half=True, conf=0.05, save_json=True,
                    save_dir=str(out))
    assert isinstance(metrics, PoseMetrics)
    v = p.validator
    ds = YOLOValDataset(tmp_path / "images" / "val", imgsz=128, batch_size=4, stride=32, num_cls=1, keypoints=True,
                        kpt_shape=(17, 3))
    hbs = list(ds.batches())
    assert len(hbs) == 1
    hb = hbs[0]
    s, det, counts, keep, kpts, _ = session_state(p)
    assert sum(counts) > 0
    H, W = hb["shape"]
    bidx = torch.from_numpy(hb["batch_idx"]).long()
    gk = torch.from_numpy(hb["keypoints"]).clone()
    pk = kpts.clone()
    for si in range(3):
        rp, ori = hb["ratio_pad"][si], hb["ori_shape"][si]
        if (bidx == si).any():
            g = gk[bidx == si]
            g[..., 0] *= W
            g[..., 1] *= H
            gk[bidx == si] = P.scale_coords((H, W), g, ori, ratio_pad=rp)
        pk[si] = P.scale_coords((H, W), pk[si].clone(), ori, ratio_pad=rp)
    boxes = native_labels(hb)
    cls = torch.from_numpy(hb["cls"]).float()
    want = P.tp_p_ref(det, counts, pk, gk, boxes, cls, bidx, P.OKS_SIGMA)
    ref = P.oks_ref(pk, counts, gk, boxes, bidx, P.OKS_SIGMA, torch.float64)
    assert P.threshold_margin(ref, cls, bidx, det, counts) >= 1e-4
    assert same_blocks(v.stats["tp_p"], want)
    assert sum(len(t) for t in v.stats["tp_p"]) == sum(counts)
    rows = json.loads((out / "predictions.json").read_text())
    assert len(rows) == sum(counts) and all(len(r["keypoints"]) == 51 for r in rows)
    first = next(si for si in range(3) if counts[si])
    assert rows[0]["keypoints"] == pytest.approx(pk[first, 0].reshape(-1).tolist())


def test_augment_warns_and_guards_raise(pairs):
    import ydbl.nn.tasks as nt

    p, _, _ = pairs("yolo11")
    x = images((96, 160))
    nt._SEG_AUGMENT_WARNED = False
    with pytest.warns(UserWarning, match="augment=True"):
        res = p.predict(x.cuda(), conf=CONF, half=True, augment=True)
    plain = p.predict(x.cuda(), conf=CONF, half=True)
    assert all(torch.equal(a.boxes.data, b.boxes.data) and torch.equal(a.keypoints.data, b.keypoints.data)
               for a, b in zip(res, plain))  # the plain pass
    nt._SEG_AUGMENT_WARNED = False
    with pytest.warns(UserWarning, match="augment=True"):
        ycat, _ = p.model(x.cuda(), augment=True)
    assert ycat.shape[1] == 4 + 1 + 51
    with pytest.raises(NotImplementedError, match="fp8"):
        p.predict(x.cuda(), fp8=True)
    batch = {"img": x, "bboxes": torch.zeros(0, 4), "cls": torch.zeros(0), "batch_idx": torch.zeros(0)}
    with pytest.raises(NotImplementedError, match="v8PoseLoss"):
        p.val([batch], loss=True)
    with pytest.raises(NotImplementedError, match="v8PoseLoss"):
        p.model.loss({"img": x.cuda(), "batch_idx": torch.zeros(0), "cls": torch.zeros(0, 1),
                      "bboxes": torch.zeros(0, 4)})
    assert len(list(p.embed(x.cuda(), half=True))) == 2  # embed: the plan never reaches the head
