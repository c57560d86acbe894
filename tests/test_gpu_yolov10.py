"""The YOLOv10 baseline on the MI355X: SCDown, RepVGGDW, CIB (lk True / False), C2fCIB and PSA at module level, and
yolov10n end to end, against the restatement of tests/yolov10_util.py.

Module level: the fused restatement (RepVGGDW folded as the reference's fuse() folds it) in fp64; bound: 2 x the
torch-CPU leg of the same precision's max deviation from fp64 + one roundoff of max|y| (a2c2f_util.leg_bound), as
tests/test_gpu_yolo11.py.  PSA's q / k rows are scaled until the softmax matters (yolo11_util.sharpen_).  End to end:
the dense one2one map (xyxy rows) under parity_util's fp32_rule / fp16_rule with the restatement's own legs -- and,
a separate claim, det / count EXACTLY equal to the pinned-order selection applied to the device's own dense map."""

import warnings

import pytest
import torch

import yolo11_util as U11
import yolov10_util as U

pytestmark = pytest.mark.gpu

MODULES = {
    "SCDown": ("SCDown", (64, 128, 3, 2), 64),
    "RepVGGDW": ("RepVGGDW", (128,), 128),
    "CIB_lk": ("CIB", (128, 128, True, 1.0, True), 128),
    "CIB": ("CIB", (128, 128, True, 1.0, False), 128),
    "CIB_64": ("CIB", (32, 32, True, 1.0, True), 32),  # 64 pointwise outputs: the fused depthwise -> pointwise launch
    "C2fCIB": ("C2fCIB", (256, 256, 2, True, True), 256),
    "PSA": ("PSA", (256, 256), 256),
}


@pytest.fixture(scope="module")
def module_case():
    """name -> (product module, x, (y64, y32, y16), peaks); built once, left unchanged."""
    from ydbl.nn import modules as M
    from ydbl.utils.synthetic import trained_like_

    cache = {}

    def get(name):
        if name not in cache:
            cls, args, c = MODULES[name]
            torch.manual_seed(0)
            o = trained_like_(getattr(U, cls)(*args).eval(), 0)
            x = torch.randn(2, c, 20, 20, generator=torch.Generator().manual_seed(11))
            peaks = U11.sharpen_(o, x) if name == "PSA" else []
            p = getattr(M, cls)(*args)
            p.load_state_dict(o.state_dict(), strict=True)
            cache[name] = (p.cuda().eval(), x, U.legs(U.fuse_module(o), x), peaks)
        return cache[name]

    return get


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("name", list(MODULES))
def test_module_forward(module_case, name, half):
    p, x, (y64, y32, y16), peaks = module_case(name)
    if name == "PSA":
        assert min(peaks) >= 0.2, peaks
    leg = y16 if half else y32
    bound = U.leg_bound(leg, y64, half)
    got = p(x.cuda().half() if half else x.cuda())
    torch.cuda.synchronize()
    assert got.dtype == (torch.float16 if half else torch.float32) and got.shape == y64.shape
    d = (got.cpu().double() - y64).abs().max().item()
    e = (leg.double() - y64).abs().max().item()
    print(f"{name} {'half' if half else 'fp32'}: max|y|={y64.abs().max():.3g} cpu leg e={e:.3g} gpu d={d:.3g} "
          f"bound={bound:.3g}")
    whats = [st.what for mp in p._fwd_plans.values() for st in mp.plan.steps]
    assert not any(w.startswith("torch.") or w == "copy" for w in whats)
    n7 = sum(w in ("RepVGGDW.dw7", "CIB.dw+pw.k7s1") for w in whats) // len(p._fwd_plans)
    assert n7 == {"RepVGGDW": 1, "CIB_lk": 1, "CIB_64": 1, "C2fCIB": 2}.get(name, 0), whats
    assert ("PSA.attn" in whats) == (name == "PSA")
    assert d <= bound


# ----------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def pairs():
    cache = {}

    def get(nc):
        if nc not in cache:
            cache[nc] = U.build_pair("n", nc)
        return cache[nc]

    return get


@pytest.fixture(scope="module")
def e2e_ref(pairs):
    """(nc, (H, W)) -> (x, the restatement's dense legs, their err_stats); computed once per model and shape."""
    from parity_util import err_stats, oracle_legs

    cache = {}

    def get(nc, hw):
        if (nc, hw) not in cache:
            x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[1]))
            ys, _ = oracle_legs(pairs(nc)[1], x, legs=("fp64", "fp32", "fp16"))
            cache[(nc, hw)] = (x, ys, {k: err_stats(ys[k], ys["fp64"]) for k in ("fp32", "fp16")})
        return cache[(nc, hw)]

    return get


def _selection_matches(s, conf, classes=None, clip=True):
    """det / count of session s == the pinned selection applied to the device's own dense map, exactly."""
    pred, det, cnt = s.pred.cpu(), s.det.cpu(), s.count.cpu()
    A = pred.shape[2]
    for b in range(pred.shape[0]):
        want = U.select_pinned(pred[b, :4].T, pred[b, 4:].T.contiguous(), k_head=min(300, A), conf=conf,
                               max_det=s.max_det, classes=classes, clip=(s.h, s.w) if clip else None)
        n = int(cnt[b])
        assert n == len(want), (b, n, len(want))
        assert torch.equal(det[b, :n], want), b
        assert not det[b, n:].any()
    return int(cnt.sum())


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("hw", [(128, 128), (96, 160)], ids=["128x128", "96x160"])
@pytest.mark.parametrize("nc", [3, 80])
def test_e2e_n(pairs, e2e_ref, nc, hw, half):
    from parity_util import err_stats, fp16_rule, fp32_rule

    p, _ = pairs(nc)
    x, ys, st_ref = e2e_ref(nc, hw)
    conf = float(ys["fp64"][:, 4:].amax(1).median())  # about half of the anchors offer a candidate
    s = p.session(2, *hw, half=half, conf=conf, keep_pred=True, use_graph=False)
    s(x.cuda())
    torch.cuda.synchronize()
    yg = s.pred.cpu()
    assert yg.shape == ys["fp64"].shape
    st = err_stats(yg, ys["fp64"])
    if half:
        tb, tc = fp16_rule(st_ref["fp16"])
        got = (st["box_p999"], st["conf_p999"])
    else:
        tb, tc = fp32_rule(st_ref["fp32"])
        got = (st["box_max"], st["conf_max"])
    print(f"yolov10n nc{nc} {hw} {'half' if half else 'fp32'}: gpu {st} | restatement leg "
          f"{st_ref['fp16' if half else 'fp32']} | bound box {tb:.3g} score {tc:.3g}")
    total = _selection_matches(s, conf)  # exactness of the selection: its own claim
    assert total > 0
    assert got[0] <= tb and got[1] <= tc


def test_selection_with_predict_settings_and_classes(pairs, e2e_ref):
    """conf 0.25-like thresholds take the one-workgroup schedule; `classes` filters behind the cut; max_det below k."""
    from ydbl import YOLO

    p0, _ = pairs(80)
    p = YOLO(str(U.GOLDEN / "yolov10n.json"), nc=80)
    p.model.load_state_dict(p0.model.state_dict(), strict=True)
    for seq in p.model.model[-1].one2one_cv3:  # class logits up by 9: the best scores pass 0.5, as after training
        seq[-1].bias.data += 9.0
    x, _, _ = e2e_ref(80, (96, 160))

    def run(classes=None, **kw):
        s = p.session(2, 96, 160, half=True, keep_pred=True, use_graph=False, classes=classes, **kw)
        s(x.cuda())
        torch.cuda.synchronize()
        n = _selection_matches(s, kw["conf"], classes)
        print(kw, classes, "->", n, "rows; candidates", s.cand_count.tolist())
        return n, s.det.cpu()

    n, det = run(conf=0.001)
    assert n == 2 * 300
    two = sorted({int(det[0, 0, 5]), int(det[0, 299, 5]), int(det[1, 150, 5])})  # classes that are in the cut
    assert run(conf=0.25)[0] > 0  # the one-workgroup schedule (conf >= 0.1)
    run(conf=0.5)
    assert run(conf=0.05, max_det=17)[0] == 2 * 17
    assert 0 < run(conf=0.25, classes=two, max_det=50)[0]
    assert 0 < run(conf=0.001, classes=two)[0] < 2 * 300


def test_plan_routing(pairs):
    """A session plan: one 7x7 depthwise launch per RepVGGDW, one PSA.attn, no torch step, no copy, NO one2many
    launch (three class tails, not six), the end2end decode and the top-k in the NMS's place."""
    from ydbl.nn import modules as M

    p, _ = pairs(3)
    s = p.session(2, 96, 160, half=True, keep_pred=True, use_graph=False)
    whats = [st.what for st in s.plan.steps]
    names = [st.fn.__name__ for st in s.plan.steps]
    reps = sum(isinstance(m, M.RepVGGDW) for m in p.model.modules())
    assert reps == 1 and whats.count("RepVGGDW.dw7") + whats.count("CIB.dw+pw.k7s1") == reps
    assert whats.count("PSA.attn") == 1 and whats.count("SPPF.pool5x3") == 1
    assert not any(w.startswith("torch.") or w == "copy" for w in whats)
    assert sum(w.startswith("DWConv+Conv1x1+1x1") or w == "Detect.cls" for w in whats) == 3
    assert names[-2:] == ["ydbl_detect_decode_e2e", "ydbl_detect_topk"] and "ydbl_nms" not in names
    assert not s.fused_candidates and not s.sparse_box


def test_streams2_bit_equal(pairs):
    p, _ = pairs(3)
    x = torch.rand(8, 3, 96, 160, generator=torch.Generator().manual_seed(8)).cuda()
    outs = []
    for streams in (1, 2):
        s = p.session(8, 96, 160, half=True, conf=0.001, keep_pred=True, use_graph=True, streams=streams)
        assert len(s.children) == (2 if streams == 2 else 0)
        s(x)
        torch.cuda.synchronize()
        outs.append((s.pred.cpu().clone(), s.det.cpu().clone(), s.count.cpu().clone()))
    assert torch.isfinite(outs[0][0]).all() and int(outs[0][2].sum()) > 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_model_forward_returns_the_reference_tuple(pairs):
    """model(x): (y [B, min(300, A), 6], {"one2many": [...], "one2one": [...]}) -- the top-k with no threshold and no
    clipping, equal to the pinned selection over the device's own one2one maps' decode."""
    p, f = pairs(3)
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(4))
    y, d = p.model(x.cuda())
    torch.cuda.synchronize()
    A = 12 * 20 + 6 * 10 + 3 * 5
    assert y.shape == (2, min(300, A), 6) and y.dtype == torch.float32
    assert sorted(d) == ["one2many", "one2one"]
    for k in d:
        assert [tuple(t.shape) for t in d[k]] == [(2, 67, 12, 20), (2, 67, 6, 10), (2, 67, 3, 5)]
    assert not torch.equal(d["one2many"][0], d["one2one"][0])
    # the same launches in a session with every pair offered and no clipping: its det is the forward's y, and the
    # pinned selection of its dense map
    s = p.session(2, 96, 160, half=False, conf=-1.0, clip=False, keep_pred=True, use_graph=False)
    s(x.cuda())
    torch.cuda.synchronize()
    assert _selection_matches(s, -1.0, clip=False) == 2 * 300
    assert torch.equal(y.cpu(), s.det.cpu())
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(d["one2one"], s.feats()))
    y2, _ = p.model(torch.rand(1, 3, 64, 64).cuda())
    assert y2.shape == (1, 84, 6)  # k_head = A below 300
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y3, _ = p.model(x.cuda(), augment=True)  # warns (once per process) and runs the plain pass
    assert torch.equal(y3, y)


def test_predict_val_track_embed(pairs):
    p, _ = pairs(3)
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(9))
    res = p.predict(x, conf=0.0, half=True)
    assert len(res) == 2
    for r in res:
        assert r.boxes.data.shape[1] == 6 and 0 < len(r.boxes) <= 300 and torch.isfinite(r.boxes.data).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        aug = p.predict(x, conf=0.0, half=True, augment=True)
    assert all(torch.equal(a.boxes.data, r.boxes.data) for a, r in zip(aug, res))
    boxes = torch.tensor([[10.0, 10.0, 60.0, 50.0], [30.0, 20.0, 120.0, 90.0], [5.0, 40.0, 70.0, 80.0]])
    batch = {"img": x, "bboxes": boxes, "cls": torch.tensor([0.0, 1.0, 2.0]), "batch_idx": torch.tensor([0, 0, 1])}
    p.val([batch], half=True)
    st = p.validator.stats
    assert len(torch.cat(st["target_cls"])) == 3 and torch.isfinite(torch.cat(st["conf"])).all()
    from track_util import CFG

    thr = float(torch.cat([r.boxes.data[:, 4] for r in res]).median())  # half of the detections can start a track
    tr = p.track(x, conf=0.0, half=True, tracker={**CFG, "fuse_score": False, "track_high_thresh": thr,
                                                  "new_track_thresh": thr, "track_low_thresh": thr / 2})
    assert len(tr) == 2
    for r in tr:
        assert r.boxes.is_track and r.boxes.id is not None and len(r.boxes.id) == len(r.boxes) > 0
        assert torch.isfinite(r.boxes.data).all()
    rows = p.embed(x, embed=[10], half=True)
    e = torch.stack(list(rows))
    assert e.shape == (2, 256) and torch.isfinite(e.float()).all()
