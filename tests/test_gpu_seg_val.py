"""val() with mask metrics on the MI355X, end to end on yolo11n-seg (and one yolov8n-seg case).

Two images per batch, 96 x 160 and 128 x 128; image 1 is flat grey and has no detection at the test's threshold
(the recipe of tests/test_gpu_seg.py).  The ground truth comes from a first predict(): label j is detection j's own
mask shifted right by a few pixels and sampled on the 1/4 grid, with the detection's box and class, drawn into the
overlap index map in label order (a later label overwrites), so the mask IoUs spread over the thresholds; one label
carries a wrong class, and image 1 has a label but no prediction.

The yardstick is SegmentationValidator._process_batch(masks=True) restated on the CPU (segval_util.tp_m_ref: the index
map's indicator, F.interpolate, > 0.5, mask_iou, oracle.metrics.match_predictions) APPLIED TO THE PRODUCT'S OWN
detections and own uint8 masks of the validated batch, so that the check is of the mask matching and not of the
network's rounding.  Compared exactly."""

import math
import warnings

import numpy as np
import pytest
import torch

import seg_util as S
import segval_util as SV

pytestmark = pytest.mark.gpu
HWS = [(96, 160), (128, 128)]


def images(hw):
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[1]))
    x[1] = 0.5
    return x


@pytest.fixture(scope="module")
def models():
    """family -> product model with the class bias shifted as in tests/test_gpu_seg.py, and (hw -> conf): between
    image 0's 6th best anchor score and the larger of its 7th and image 1's best, on the restatement's fp32 leg."""
    cache = {}

    def get(family):
        if family not in cache:
            x = images((128, 128))
            p, o = S.build_pair(family, "n", 3, x)
            with torch.no_grad():
                z = torch.logit(o(x)[0][:, 4:7].amax(1).double())
            hi, lo = z[0].topk(6).values[-1].item(), z[1].max().item()
            delta = math.log(0.25 / 0.75) - (hi + lo) / 2
            with torch.no_grad():
                for m in (p.model.model[-1], o.model[-1]):
                    for seq in m.cv3:
                        seq[-1].bias += delta
            p.reset_sessions()
            confs = {}
            for hw in HWS:
                with torch.no_grad():
                    sc = o(images(hw))[0][:, 4:7].amax(1)
                top = sc[0].topk(7).values
                floor = max(float(top[6]), float(sc[1].max()))
                assert float(top[5]) > floor
                confs[hw] = (float(top[5]) + floor) / 2
            cache[family] = (p, confs)
        return cache[family]

    return get


def make_batch(p, x, conf):
    """The ground truth of the module docstring from a predict() of the batch."""
    res = p.predict(x.cuda(), conf=conf, half=True)
    H, W = x.shape[2:]
    masks0, boxes0 = res[0].masks.data.cpu(), res[0].boxes.data.cpu().float()
    k = len(boxes0)
    assert k >= 2 and len(res[1].boxes.data) == 0
    gmap = torch.zeros(2, H // 4, W // 4, dtype=torch.uint8)
    for j in range(k):
        m = torch.roll(masks0[j], 1 + (k - 1 - j) % 6, dims=1)[::4, ::4]
        gmap[0][m != 0] = j + 1
    gmap[1, 4:12, 6:20] = 1
    cls = boxes0[:, 5].clone()
    cls[0] = (cls[0] + 1) % 3  # one label of the wrong class (the first drawn; the last one is whole)
    # image 1's label comes first in the list: the grouping by image is part of what is checked
    bboxes = torch.cat([torch.tensor([[24.0, 16.0, 80.0, 48.0]]), boxes0[:, :4]])
    return {"img": x, "bboxes": bboxes, "cls": torch.cat([torch.tensor([2.0]), cls]),
            "batch_idx": torch.tensor([1] + [0] * k), "masks": gmap}


def reference_blocks(p, batch, overlap=True):
    """tp_m of the batch the validator just scored, from its session's own det rows and uint8 masks."""
    s = p.validator._sess
    cnt = s.count.cpu().tolist()
    pm, offs = s.masks(cnt, dtype=torch.uint8)
    return SV.tp_m_ref(s.det.cpu(), cnt, pm.cpu(), offs, batch["masks"], batch["cls"], batch["batch_idx"], overlap)[0]


def same_blocks(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("family,hw", [("yolo11", HWS[0]), ("yolo11", HWS[1]), ("yolov8", HWS[0])],
                         ids=["yolo11-96x160", "yolo11-128x128", "yolov8-96x160"])
def test_val_with_masks(models, family, hw):
    import ydbl.engine.model as em
    from ydbl.utils.metrics import DetMetrics, SegmentMetrics, ap_per_class

    p, confs = models(family)
    conf, x = confs[hw], images(hw)
    batch = make_batch(p, x, conf)
    em._SEG_VAL_WARNED = False
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*mask metrics.*")
        metrics = p.val([batch], half=True, conf=conf)
    assert isinstance(metrics, SegmentMetrics) and not em._SEG_VAL_WARNED
    v = p.validator
    assert list(v.stats) == ["tp", "tp_m", "conf", "pred_cls", "target_cls"]
    want = reference_blocks(p, batch)
    got = v.stats["tp_m"]
    assert same_blocks(got, want)
    assert [tuple(g.shape) for g in got][-1] == (0, 10)  # image 1: labels, no predictions
    tp_m = torch.cat(got)
    print(f"{family} {hw}: {tp_m.shape[0]} detections, tp_m per threshold {tp_m.sum(0).tolist()}, "
          f"tp {torch.cat(v.stats['tp']).sum(0).tolist()}")
    assert tp_m.any() and not tp_m.all() and tp_m.shape == torch.cat(v.stats["tp"]).shape
    st = {k: torch.cat(t).numpy() for k, t in v.stats.items()}
    ap = ap_per_class(st["tp_m"], st["conf"], st["pred_cls"], st["target_cls"])[5]
    assert metrics.seg.map50 == float(ap[:, 0].mean()) and metrics.seg.map75 == float(ap[:, 5].mean())
    assert metrics.seg.map == float(ap.mean()) and metrics.seg.map50 > 0
    assert metrics.results_dict["metrics/mAP50(M)"] == metrics.seg.map50
    assert "Mask(P" in v.get_desc() and len(v.print_results()) >= 1
    seg_stats = {k: [t.clone() for t in ts] for k, ts in v.stats.items()}

    # overlap_mask=False: the same labels as planes, in label order
    order_cls = batch["batch_idx"]
    planes = torch.stack([batch["masks"][int(b)] == (int((order_cls[:i] == b).sum()) + 1)
                          for i, b in enumerate(order_cls)]).to(torch.uint8)
    p.val([{**batch, "masks": planes}], half=True, conf=conf, overlap_mask=False)
    assert same_blocks(p.validator.stats["tp_m"], want)

    # the box side: what the same val() gives without masks
    plain = {k: t for k, t in batch.items() if k != "masks"}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        box = p.val([plain], half=True, conf=conf)
    assert isinstance(box, DetMetrics) and "tp_m" not in p.validator.stats
    assert same_blocks(p.validator.stats["tp"], seg_stats["tp"])
    for a in ("p", "r", "f1", "all_ap", "ap_class_index"):
        assert np.array_equal(getattr(metrics.box, a), getattr(box.box, a)), a
    assert np.array_equal(metrics.confusion_matrix.matrix, box.confusion_matrix.matrix)


def test_val_masks_guards_on_the_device(models):
    p, confs = models("yolo11")
    x = images(HWS[0])
    lab = {"img": x, "bboxes": torch.zeros(0, 4), "cls": torch.zeros(0), "batch_idx": torch.zeros(0)}
    with pytest.raises(ValueError, match="index map"):
        p.val([{**lab, "masks": torch.zeros(3, 24, 40, dtype=torch.uint8)}], half=True, conf=confs[HWS[0]])
    gen = (b for b in [{**lab, "masks": torch.zeros(2, 24, 40, dtype=torch.uint8)}, lab])
    with pytest.raises(ValueError, match="only some"):
        p.val(gen, half=True, conf=confs[HWS[0]])


def test_val_dataset_with_polygons(models, tmp_path):
    """A dataset whose label files hold polygon rows: SegmentMetrics, and tp_m equal to the CPU reference fed with
    the dataset's own "masks" (one batch: the session still holds it)."""
    import dataset_util as D
    from ydbl.engine.dataset import YOLOValDataset
    from ydbl.utils.metrics import SegmentMetrics

    p, _ = models("yolo11")
    D.make_dataset(tmp_path, shapes=[(96, 128), (100, 128), (90, 120)], nc=3, labels={}, edge_cases=False)
    lb = tmp_path / "labels" / "val"
    (lb / "im000.txt").write_text("0 0.1 0.1 0.5 0.15 0.45 0.6 0.12 0.5\n1 0.2 0.2 0.9 0.2 0.9 0.9 0.2 0.9\n")
    (lb / "im001.txt").write_text("2 0.3 0.3 0.7 0.3 0.7 0.7 0.5 0.5 0.3 0.7\n1 0.5 0.5 0.2 0.2\n")
    (lb / "im002.txt").write_text("")
    metrics = p.val(data=str(tmp_path / "data.yaml"), imgsz=128, batch=4, half=True)
    assert isinstance(metrics, SegmentMetrics)
    v = p.validator
    ds = YOLOValDataset(tmp_path / "images" / "val", imgsz=128, batch_size=4, stride=32, num_cls=3, masks=True)
    hbs = list(ds.batches())
    assert len(hbs) == 1 and hbs[0]["masks"].max() >= 2
    hb = hbs[0]
    batch = {"masks": torch.from_numpy(hb["masks"]), "cls": torch.from_numpy(hb["cls"]),
             "batch_idx": torch.from_numpy(hb["batch_idx"])}
    want = reference_blocks(p, batch)
    assert same_blocks(v.stats["tp_m"], want)
    assert sum(len(t) for t in v.stats["tp_m"]) == sum(len(t) for t in v.stats["tp"]) > 0
