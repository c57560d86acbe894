"""The YOLO11 / YOLOv8 baselines on the MI355X: SPPF, C3k2, PSABlock and C2PSA at module level, and yolo11n / yolov8n
end to end, against the restatement of tests/yolo11_util.py.

Module level: q / k rows of every qkv are scaled until the fp64 restatement's mean row-maximum softmax probability is
>= 0.2 (asserted: with init weights the softmax is uniform and the attention kernel would not matter), v rows and
proj x 8.  Bound: 2 x the torch-CPU leg of the same precision's max deviation from fp64 + one roundoff of max|y|
(a2c2f_util.leg_bound).  End to end the init weights make it a routing test (SPPF's and C2PSA's buffers, C3k2 chains,
Detect legacy True / False); bounds: parity_util's fp32_rule / fp16_rule with the restatement's own legs."""

import pytest
import torch

import yolo11_util as U

pytestmark = pytest.mark.gpu

MODULES = {
    "SPPF": ("SPPF", (256, 256, 5), 256, ["SPPF.pool5x3"]),
    "C3k2": ("C3k2", (128, 256, 2, False, 0.25), 128, ["Conv3x3"]),
    "C3k2_c3k": ("C3k2", (256, 256, 1, True), 256, ["Conv1x1x2"]),
    "PSABlock": ("PSABlock", (128, 0.5, 2), 128, ["PSA.attn"]),
    "C2PSA": ("C2PSA", (256, 256, 2), 256, ["PSA.attn", "PSA.attn"]),
}
ATTN = ("PSABlock", "C2PSA")


@pytest.fixture(scope="module")
def module_case():
    """name -> (product module, x, (y64, y32, y16), peaks); built once, left unchanged."""
    from ydbl.nn import modules as M
    from ydbl.utils.synthetic import trained_like_

    cache = {}

    def get(name):
        if name not in cache:
            cls, args, c, _ = MODULES[name]
            torch.manual_seed(0)
            o = trained_like_(getattr(U, cls)(*args).eval(), 0)
            x = torch.randn(2, c, 20, 20, generator=torch.Generator().manual_seed(11))
            peaks = U.sharpen_(o, x) if name in ATTN else []
            p = getattr(M, cls)(*args)
            p.load_state_dict(o.state_dict(), strict=True)
            cache[name] = (p.cuda().eval(), x, U.legs(U.fuse_(o), x), peaks)
        return cache[name]

    return get


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("name", list(MODULES))
def test_module_forward(module_case, name, half):
    p, x, (y64, y32, y16), peaks = module_case(name)
    if name in ATTN:
        assert min(peaks) >= 0.2, peaks
    leg = y16 if half else y32
    bound = U.leg_bound(leg, y64, half)
    got = p(x.cuda().half() if half else x.cuda())
    torch.cuda.synchronize()
    assert got.dtype == (torch.float16 if half else torch.float32) and got.shape == y64.shape
    d = (got.cpu().double() - y64).abs().max().item()
    e = (leg.double() - y64).abs().max().item()
    print(f"{name} {'half' if half else 'fp32'}: peaks {[round(v, 3) for v in peaks]} max|y|={y64.abs().max():.3g} "
          f"cpu leg e={e:.3g} gpu d={d:.3g} bound={bound:.3g}")
    whats = [st.what for mp in p._fwd_plans.values() for st in mp.plan.steps]
    for w in set(MODULES[name][3]):
        assert whats.count(w) >= MODULES[name][3].count(w), whats
    assert ("SPPF.pool5x3" in whats) == (name == "SPPF")
    assert ("PSA.attn" in whats) == (name in ATTN)
    assert d <= bound


def test_psablock_without_shortcut(module_case):
    """PSABlock(shortcut=False): no residual rides in proj's or ffn[1]'s epilogue; fp32 against its own legs."""
    from ydbl.nn import modules as M
    from ydbl.utils.synthetic import trained_like_

    torch.manual_seed(0)
    o = trained_like_(U.PSABlock(128, 0.5, 2, False).eval(), 0)
    x = torch.randn(2, 128, 20, 20, generator=torch.Generator().manual_seed(11))
    peaks = U.sharpen_(o, x)
    assert min(peaks) >= 0.2, peaks
    p = M.PSABlock(128, 0.5, 2, False)
    p.load_state_dict(o.state_dict(), strict=True)
    y64, y32, _ = U.legs(U.fuse_(o), x)
    got = p.cuda().eval()(x.cuda())
    torch.cuda.synchronize()
    d = (got.cpu().double() - y64).abs().max().item()
    bound = U.leg_bound(y32, y64, False)
    print(f"PSABlock shortcut=False fp32: gpu d={d:.3g} bound={bound:.3g}")
    assert d <= bound


# ----------------------------------------------------------------------------------------------- end to end
FAMILIES = ["yolo11", "yolov8"]


@pytest.fixture(scope="module")
def pairs():
    cache = {}

    def get(family):
        if family not in cache:
            cache[family] = U.build_pair(family, "n", 3)
        return cache[family]

    return get


@pytest.fixture(scope="module")
def e2e_ref(pairs):
    """(family, (H, W)) -> (x, the restatement's legs, their err_stats); computed once per model and shape."""
    from parity_util import err_stats, oracle_legs

    cache = {}

    def get(family, hw):
        if (family, hw) not in cache:
            x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[1]))
            ys, _ = oracle_legs(pairs(family)[1], x, legs=("fp64", "fp32", "fp16"))
            cache[(family, hw)] = (x, ys, {k: err_stats(ys[k], ys["fp64"]) for k in ("fp32", "fp16")})
        return cache[(family, hw)]

    return get


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("hw", [(128, 128), (96, 160)], ids=["128x128", "96x160"])
@pytest.mark.parametrize("family", FAMILIES)
def test_e2e_n(pairs, e2e_ref, family, hw, half):
    """96x160: a 3x5 P5 map -- 15 attention tokens, a pool window larger than the map."""
    from parity_util import err_stats, fp16_rule, fp32_rule, gpu_pred

    p, _ = pairs(family)
    x, ys, st_ref = e2e_ref(family, hw)
    yg, _ = gpu_pred(p, x, half=half)
    assert yg.shape == ys["fp64"].shape
    st = err_stats(yg, ys["fp64"])
    if half:
        tb, tc = fp16_rule(st_ref["fp16"])
        got = (st["box_p999"], st["conf_p999"])
    else:
        tb, tc = fp32_rule(st_ref["fp32"])
        got = (st["box_max"], st["conf_max"])
    print(f"{family}n {hw} {'half' if half else 'fp32'}: gpu {st} | restatement leg "
          f"{st_ref['fp16' if half else 'fp32']} | bound box {tb:.3g} score {tc:.3g}")
    assert got[0] <= tb and got[1] <= tc


def test_e2e_plan_routing(pairs):
    """yolo11n: one SPPF = one pool launch, and one attention launch per PSABlock of the model (at scale n the depth
    rule leaves C2PSA's two repeats as max(round(2 * 0.5), 1) = 1 block; the count is taken from the model);
    yolov8n: one pool launch, no attention.  Neither plan holds an eager torch step or a concat copy."""
    from ydbl.nn import modules as M

    p, _ = pairs("yolo11")
    s = p.session(2, 96, 160, half=True, keep_pred=True, use_graph=False)
    whats = [st.what for st in s.plan.steps]
    blocks = sum(isinstance(m, M.PSABlock) for m in p.model.modules())
    assert sum(isinstance(m, M.SPPF) for m in p.model.modules()) == 1 and blocks >= 1
    assert whats.count("SPPF.pool5x3") == 1
    assert whats.count("PSA.attn") == blocks
    assert whats.count("Upsample.nearest2") == 2
    assert not any(w.startswith("torch.") or w == "copy" for w in whats)  # no eager step, no concat copy
    p8, _ = pairs("yolov8")
    s8 = p8.session(2, 96, 160, half=True, keep_pred=True, use_graph=False)
    w8 = [st.what for st in s8.plan.steps]
    assert w8.count("SPPF.pool5x3") == 1 and "PSA.attn" not in w8
    assert not any(w.startswith("torch.") or w == "copy" for w in w8)


def test_routing_two_psablocks():
    """The issue's count -- one SPPF, two PSABlocks -- holds where C2PSA's two repeats survive the depth rule (l);
    checked on a meta plan of the C2PSA layer alone at depth 1: C2PSA(256, 256, 2)."""
    from ydbl.nn import modules as M
    from ydbl.runtime import Plan

    plan = Plan(torch.device("meta"), torch.float16)
    m = M.C2PSA(256, 256, 2)
    m.emit(plan, plan.alloc(2, 20, 20, 256))
    whats = [st.what for st in plan.steps]
    assert whats.count("PSA.attn") == 2 and len(m.m) == 2


@pytest.mark.parametrize("family", FAMILIES)
def test_e2e_streams2_bit_equal(pairs, family):
    p, _ = pairs(family)
    x = torch.rand(8, 3, 96, 160, generator=torch.Generator().manual_seed(8)).cuda()
    outs = []
    for streams in (1, 2):
        s = p.session(8, 96, 160, half=True, keep_pred=True, use_graph=True, streams=streams)
        assert len(s.children) == (2 if streams == 2 else 0)
        s(x)
        torch.cuda.synchronize()
        outs.append(s.pred.cpu().clone())
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_predict_augment_returns_boxes(pairs):
    p, _ = pairs("yolo11")
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(9))
    res = p.predict(x, augment=True, conf=0.001, half=True)
    assert len(res) == 2
    for r in res:
        assert r.boxes.data.shape[1] == 6 and len(r.boxes) > 0 and torch.isfinite(r.boxes.data).all()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_val_runs(pairs, half):
    """val() on a tensor batch with made-up labels runs on yolo11n in both precisions (the validation session --
    multi-label NMS, matching, the report -- builds and runs on this model)."""
    p, _ = pairs("yolo11")
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(10))
    boxes = torch.tensor([[10.0, 10.0, 60.0, 50.0], [30.0, 20.0, 120.0, 90.0], [5.0, 40.0, 70.0, 80.0]])
    batch = {"img": x, "bboxes": boxes, "cls": torch.tensor([0.0, 1.0, 2.0]), "batch_idx": torch.tensor([0, 0, 1])}
    p.val([batch], half=half)
    st = p.validator.stats
    assert len(torch.cat(st["target_cls"])) == 3
    assert torch.isfinite(torch.cat(st["conf"])).all()


def test_embed_layer_10(pairs):
    """embed=[10]: C2PSA's pooled output, 256 channels at scale n."""
    p, _ = pairs("yolo11")
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(12))
    rows = p.embed(x, embed=[10], half=True)
    e = torch.stack(list(rows))
    assert e.shape == (2, 256) and torch.isfinite(e.float()).all()
