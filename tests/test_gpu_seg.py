"""The segmentation models on the MI355X: Proto and Segment at module level, yolo11n-seg / yolov8n-seg end to end.

Module level: the product module's forward against the fp64 leg of the restatement (tests/seg_util.py) under
a2c2f_util.leg_bound, with the torch-CPU leg of the same precision as the yardstick; Proto's plan must hold exactly one
deconv2x2 launch.  End to end (128^2 and 96 x 160, nc 3, trained-like BN): model(x) has the reference's shapes and y,
mc, p lie within parity_util's fp32_rule / fp16_rule of the restatement's legs; predict()'s boxes are the detection
twin's (the same weights under a Detect head) bit for bit; the masks equal the restatement's process_mask /
process_mask_native FED THE DEVICE'S OWN det rows, coefficients and prototypes (the rule of tests/test_gpu_mask.py), so
that the check is of the mask path and not of the network's rounding.  The weights are scaled so that the prediction
depends on the image (seg_util.sensitize_), and the class bias is shifted so that at 128^2 image 0 has detections at
conf 0.25 and image 1 (a flat grey image) has none; at 96 x 160 the threshold is put under image 0's 6th best anchor."""

import math
import warnings

import pytest
import torch

import seg_util as S

pytestmark = pytest.mark.gpu
FAMILIES = ["yolo11", "yolov8"]
CONF = 0.25
HWS = [(128, 128), (96, 160)]


# ----------------------------------------------------------------------------------------------- module level
@pytest.fixture(scope="module")
def proto_case():
    from ydbl.nn import modules as M
    from ydbl.utils.synthetic import trained_like_

    torch.manual_seed(0)
    o = trained_like_(S.Proto(64, 64, 32).eval(), 0)
    x = torch.randn(2, 64, 20, 20, generator=torch.Generator().manual_seed(11))
    p = M.Proto(64, 64, 32)
    p.load_state_dict(o.state_dict(), strict=True)
    return p.cuda().eval(), x, S.legs(S.fuse_(o), x)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_proto_forward(proto_case, half):
    p, x, (y64, y32, y16) = proto_case
    leg = y16 if half else y32
    got = p(x.cuda().half() if half else x.cuda())
    torch.cuda.synchronize()
    assert got.dtype == (torch.float16 if half else torch.float32) and got.shape == y64.shape == (2, 32, 40, 40)
    d = (got.cpu().double() - y64).abs().max().item()
    bound = S.leg_bound(leg, y64, half)
    print(f"Proto {'half' if half else 'fp32'}: max|y|={y64.abs().max():.3g} gpu d={d:.3g} bound={bound:.3g}")
    for mp in p._fwd_plans.values():
        assert [st.what for st in mp.plan.steps].count("deconv2x2") == 1
    assert d <= bound


@pytest.fixture(scope="module")
def segment_case():
    from ydbl.nn import modules as M
    from ydbl.utils.synthetic import trained_like_

    ch = (64, 128, 256)  # the three n-scale level shapes at 64^2
    torch.manual_seed(0)
    o = S.Segment(3, 32, 64, ch, legacy=False).eval()
    o.stride = torch.tensor([8.0, 16.0, 32.0])
    o.bias_init()
    trained_like_(o, 0)
    g = torch.Generator().manual_seed(13)
    xs = [torch.randn(2, c, 64 // s, 64 // s, generator=g) for c, s in zip(ch, (8, 16, 32))]
    p = M.Segment(3, 32, 64, ch, legacy=False)
    p.stride = o.stride.clone()
    p.load_state_dict(o.state_dict(), strict=True)
    f = S.fuse_(o)
    with torch.no_grad():
        outs = [f.double()([x.double() for x in xs]), None, None]
        f = f.float()
        outs[1] = f(xs)
        outs[2] = f.half()([x.half() for x in xs])
    return p.cuda().eval(), xs, outs


def _flat(out):
    ycat, (feats, mc, pr) = out
    return {"ycat": ycat, "mc": mc, "p": pr, **{f"feat{i}": f for i, f in enumerate(feats)}}


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_segment_forward(segment_case, half):
    p, xs, (o64, o32, o16) = segment_case
    got = _flat(p([x.cuda().half() if half else x.cuda() for x in xs]))
    torch.cuda.synchronize()
    ref, leg = _flat(o64), _flat(o16 if half else o32)
    A = 64 + 16 + 4
    assert got["ycat"].shape == (2, 4 + 3 + 32, A) and got["mc"].shape == (2, 32, A)
    assert got["p"].shape == (2, 32, 16, 16)
    assert torch.equal(got["ycat"][:, 7:], got["mc"])
    for k in ref:
        assert got[k].shape == ref[k].shape, k
        d = (got[k].cpu().double() - ref[k]).abs().max().item()
        bound = S.leg_bound(leg[k], ref[k], half)
        print(f"Segment {'half' if half else 'fp32'} {k}: gpu d={d:.3g} bound={bound:.3g}")
        assert d <= bound, k


# ----------------------------------------------------------------------------------------------- end to end
def _logit(v):
    return math.log(v / (1 - v))


@pytest.fixture(scope="module")
def pairs():
    """family -> (product, fused restatement, detection twin): the class bias of all three shifted by one constant so
    that, on the 128^2 test batch, image 0's 6th best anchor scores above CONF and image 1's best below it (the two
    sit at equal distance from the threshold in logits)."""
    from ydbl import YOLO

    cache = {}

    def get(family):
        if family not in cache:
            x = images((128, 128))
            p, o = S.build_pair(family, "n", 3, x)
            with torch.no_grad():
                z = torch.logit(o(x)[0][:, 4:7].amax(1).double())  # best class logit per anchor
            hi, lo = z[0].topk(6).values[-1].item(), z[1].max().item()
            assert hi - lo > 0.2, (hi, lo)  # far more than the fp16 noise of a logit
            delta = _logit(CONF) - (hi + lo) / 2
            with torch.no_grad():
                for m in (p.model.model[-1], o.model[-1]):
                    for seq in m.cv3:
                        seq[-1].bias += delta
            p.reset_sessions()
            twin = YOLO(str(S.GOLDEN / f"{family}n.json"), nc=3)
            twin.model.load_state_dict({k: v for k, v in p.model.state_dict().items()
                                        if ".proto." not in k and ".cv4." not in k}, strict=True)
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
                sc = pairs(family)[1](images(hw))[0][0, 4:7].amax(0).topk(7).values
            cache[(family, hw)] = float((sc[5] + sc[6]) / 2)
        return cache[(family, hw)]

    return get


def images(hw):
    """Image 0 random, image 1 flat grey: their best class scores differ by a wide margin."""
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[1]))
    x[1] = 0.5
    return x


def dev_stats(t, t64):
    d = (t.double() - t64).abs().flatten()
    q = torch.quantile(d[torch.randperm(d.numel(), generator=torch.Generator().manual_seed(0))[:1 << 20]], 0.999)
    return {"box_max": d.max().item(), "box_p999": q.item(), "conf_max": 0.0, "conf_p999": 0.0}


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("hw", HWS, ids=["128x128", "96x160"])
@pytest.mark.parametrize("family", FAMILIES)
def test_model_forward(pairs, family, hw, half):
    import copy

    from parity_util import err_stats, fp16_rule, fp32_rule

    p, o, _ = pairs(family)
    x = images(hw)
    with torch.inference_mode():
        r64 = copy.deepcopy(o).double()(x.double())
        rleg = copy.deepcopy(o).half()(x.half()) if half else o(x)
    ycat, (feats, mc, pr) = p.model(x.cuda().half() if half else x.cuda())
    torch.cuda.synchronize()
    A = sum((hw[0] // s) * (hw[1] // s) for s in (8, 16, 32))
    assert ycat.shape == (2, 4 + 3 + 32, A) and mc.shape == (2, 32, A) and pr.shape == (2, 32, hw[0] // 4, hw[1] // 4)
    assert [tuple(f.shape) for f in feats] == [(2, 67, hw[0] // s, hw[1] // s) for s in (8, 16, 32)]
    assert ycat.dtype == mc.dtype == pr.dtype == (torch.float16 if half else torch.float32)
    assert torch.equal(ycat[:, 7:], mc)
    rule, key = (fp16_rule, "box_p999") if half else (fp32_rule, "box_max")
    st, st_ref = err_stats(ycat[:, :7].cpu(), r64[0][:, :7]), err_stats(rleg[0][:, :7].float(), r64[0][:, :7])
    tb, tc = rule(st_ref)
    print(f"{family}n-seg {hw} {'half' if half else 'fp32'} y: gpu {st} | leg {st_ref}")
    assert st[key] <= tb and st[key.replace("box", "conf")] <= tc
    for name, got, ref, leg in (("mc", mc, r64[1][1], rleg[1][1]), ("p", pr, r64[1][2], rleg[1][2])):
        sg, sl = dev_stats(got.cpu(), ref), dev_stats(leg.float(), ref)
        print(f"{family}n-seg {hw} {'half' if half else 'fp32'} {name}: gpu {sg[key]:.3g} leg {sl[key]:.3g} "
              f"bound {rule(sl)[0]:.3g}")
        assert sg[key] <= rule(sl)[0], name


def device_state(p):
    """The most recently used session's det rows, kept indices, coefficients and prototypes, on the host."""
    s = list(p._sessions.values())[-1]
    mc, pr = s.seg_outputs()
    keep = torch.cat([part.keep_idx for part in s.parts])
    torch.cuda.synchronize()
    return s.det.cpu(), s.count.cpu().tolist(), keep.cpu(), mc.float().cpu(), pr.cpu()


def check_masks(results, p, form, frames=None):
    """Every image's masks against the restatement fed the device's own values; returns the detection counts."""
    det, counts, keep, mc, pr = device_state(p)
    near_tot = pos_tot = 0
    for i, r in enumerate(results):
        k = counts[i]
        assert len(r.boxes) == k
        if k == 0:
            assert r.masks is None
            continue
        m = r.masks.data
        assert len(r.masks) == k and ((m == 0) | (m == 1)).all()
        assert (keep[i, :k] >= 0).all() and (keep[i, k:] == -1).all()
        coef = mc[i][:, keep[i, :k].long()].t().contiguous()
        proto = pr[i]
        if form == "up":
            h, w = 4 * proto.shape[1], 4 * proto.shape[2]
            assert m.shape[1:] == (h, w)
            v64 = S.process_mask(proto, coef, det[i, :k, :4], (h, w), True, torch.float64, False)
            s64 = S.process_mask(proto.abs(), coef.abs(), det[i, :k, :4], (h, w), True, torch.float64, False)
        else:
            shape = tuple(frames[i]) if frames is not None else (4 * proto.shape[1], 4 * proto.shape[2])
            assert m.shape[1:] == shape and r.masks.orig_shape == shape
            boxes = r.boxes.data[:, :4].cpu().float()
            v64 = S.process_mask_native(proto, coef, boxes, shape, torch.float64, False)
            s64 = S.process_mask_native(proto.abs(), coef.abs(), boxes, shape, torch.float64, False)
        wrong, near, pos = S.mask_check(m.cpu(), v64, s64)
        assert wrong == 0, (i, wrong)
        assert m.sum() > 0  # some mask has pixels: an all-zero output would pass the S == 0 half of the rule
        near_tot, pos_tot = near_tot + near, pos_tot + pos
    assert near_tot <= S.NEAR_ZERO_CAP * max(pos_tot, 1)
    print(f"masks {form}: counts {counts}, near-zero {near_tot} / {pos_tot}")
    return counts


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("hw", HWS, ids=["128x128", "96x160"])
@pytest.mark.parametrize("family", FAMILIES)
def test_predict_boxes_and_masks(pairs, conf_of, family, hw, half):
    p, _, twin = pairs(family)
    x = images(hw).cuda()
    conf = conf_of(family, hw)
    res = p.predict(x, conf=conf, half=half)
    counts = check_masks(res, p, "up")
    assert counts[0] > 0
    if hw == (128, 128):  # the batch the bias was set on: detections in image 0, none in image 1
        assert counts[1] == 0 and res[1].masks is None
    assert res[0].masks.data.dtype == torch.float32
    det_res = twin.predict(x, conf=conf, half=half)
    for a, b in zip(res, det_res):
        assert torch.equal(a.boxes.data, b.boxes.data)  # the box path is the detection path's
        assert b.masks is None
    u8 = p.predict(x, conf=conf, half=half, mask_dtype=torch.uint8)
    assert u8[0].masks.data.dtype == torch.uint8 and torch.equal(u8[0].masks.data.float(), res[0].masks.data)
    if hw == (128, 128):  # batch 4: two sub-batch plans, one mask launch each, into one [sum(count), h, w] tensor
        four = p.predict(torch.cat([x, x]), conf=conf, half=half)
        assert len(list(p._sessions.values())[-1].children) == 2
        assert torch.equal(four[0].masks.data, res[0].masks.data) and torch.equal(four[2].masks.data, res[0].masks.data)
        assert four[1].masks is None and four[3].masks is None
        assert torch.equal(four[2].boxes.data, res[0].boxes.data)
    assert len(res[0][:1].masks) == 1 and res[0].cpu().masks.data.device.type == "cpu"


@pytest.mark.parametrize("family", FAMILIES)
def test_retina_masks_tensor_source(pairs, family):
    p, _, _ = pairs(family)
    x = images((128, 128)).cuda()
    res = p.predict(x, conf=CONF, half=True, retina_masks=True)
    counts = check_masks(res, p, "native")
    assert counts[0] > 0 and counts[1] == 0
    plain = p.predict(x, conf=CONF, half=True)
    assert torch.equal(plain[0].boxes.data, res[0].boxes.data)


def test_retina_masks_image_files(pairs, tmp_path):
    """Two image files of different shapes in one batch: masks at each original shape, one launch per image."""
    from PIL import Image

    p, _, _ = pairs("yolo11")
    g = torch.Generator().manual_seed(3)
    shapes = [(150, 200), (190, 120)]
    paths = []
    for i, (h, w) in enumerate(shapes):
        a = (torch.rand(h, w, 3, generator=g) * 255).byte().numpy()
        paths.append(str(tmp_path / f"im{i}.png"))
        Image.fromarray(a).save(paths[-1])
    res = p.predict(paths, conf=0.05, half=True, retina_masks=True, imgsz=128, batch=2)
    counts = check_masks(res, p, "native", frames=shapes)
    assert sum(counts) > 0
    for r, shp in zip(res, shapes):
        assert r.orig_shape == shp
    plain = p.predict(paths, conf=0.05, half=True, imgsz=128, batch=2)  # masks at the letterboxed size
    for r in plain:
        if r.masks is not None:
            assert r.masks.data.shape[1] % 32 == 0 and r.masks.data.shape[2] % 32 == 0


def test_track_carries_masks(pairs):
    p, _, _ = pairs("yolo11")
    x = images((128, 128)).cuda()
    pred = p.predict(x, conf=CONF, half=True)
    res = p.track(x, conf=CONF, half=True)
    assert len(res[0].boxes) > 0 and res[1].masks is None and len(res[1].boxes) == 0
    m = res[0].masks.data
    assert len(res[0].masks) == len(res[0].boxes) and m.shape[1:] == (128, 128)
    pool = pred[0].masks.data
    if res[0].boxes.is_track:  # each track's mask is the mask of the detection it was matched to
        assert res[0].boxes.data.shape[1] == 7
    for j in range(len(m)):
        assert any(torch.equal(m[j], pool[q]) for q in range(len(pool)))


def test_val_and_augment_warn(pairs):
    import ydbl.engine.model as em
    import ydbl.nn.tasks as nt

    p, _, _ = pairs("yolo11")
    x = images((96, 160))
    boxes = torch.tensor([[10.0, 10.0, 60.0, 50.0], [30.0, 20.0, 120.0, 90.0], [5.0, 40.0, 70.0, 80.0]])
    batch = {"img": x, "bboxes": boxes, "cls": torch.tensor([0.0, 1.0, 2.0]), "batch_idx": torch.tensor([0, 0, 1])}
    em._SEG_VAL_WARNED = False
    with pytest.warns(UserWarning, match="mask metrics"):
        metrics = p.val([batch], half=True)
    assert metrics is not None and len(torch.cat(p.validator.stats["target_cls"])) == 3
    with warnings.catch_warnings():  # said once
        warnings.simplefilter("error")
        em._warn_seg_val()
    nt._SEG_AUGMENT_WARNED = False
    with pytest.warns(UserWarning, match="augment=True"):
        res = p.predict(x.cuda(), conf=CONF, half=True, augment=True)
    plain = p.predict(x.cuda(), conf=CONF, half=True)
    assert all(torch.equal(a.boxes.data, b.boxes.data) for a, b in zip(res, plain))  # the plain pass
    nt._SEG_AUGMENT_WARNED = False
    with pytest.warns(UserWarning, match="augment=True"):
        ycat, _ = p.model(x.cuda(), augment=True)
    assert ycat.shape[1] == 4 + 3 + 32
    assert len(list(p.embed(x.cuda(), half=True))) == 2  # embed: the plan never reaches the head
