"""The YOLOv13 baseline on the MI355X: the A2C2f family at module level, grouped Conv, nn.Upsample into a concat
slice, and yolov13n end to end, against the restatement of tests/a2c2f_util.py.

Module level: q / k rows of every qkv are scaled until the fp64 restatement's mean row-maximum softmax probability is
>= 0.2 (asserted: with init weights the softmax is uniform and the attention kernel would not matter), v rows and
proj x 8.  Bound: 2 x the torch-CPU leg of the same precision's max deviation from fp64 + one roundoff of max|y|.
End to end the init weights make it a routing test (concat slices, FullPAD fusions around grouped and upsampled
producers, Detect legacy=False); bounds: parity_util's fp32_rule / fp16_rule with the restatement's own legs."""

import pytest
import torch
import torch.nn.functional as F

import a2c2f_util as U

pytestmark = pytest.mark.gpu

MODULES = {
    "AAttn": ("AAttn", (64, 2, 4), 64),
    "ABlock": ("ABlock", (128, 4, 1.2, 1), 128),
    "A2C2f": ("A2C2f", (128, 128, 2, True, 4), 128),
    "A2C2f_gamma": ("A2C2f", (256, 256, 1, True, 4, True, 1.5), 256),
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
            if getattr(o, "gamma", None) is not None:
                with torch.no_grad():  # 0.01 at init: make the gated branch count, channel by channel
                    o.gamma.copy_(torch.linspace(0.25, 1.0, o.gamma.numel()))
            peaks = U.sharpen_(o, x)
            p = getattr(M, cls)(*args)
            p.load_state_dict(o.state_dict(), strict=True)
            cache[name] = (p.cuda().eval(), x, U.legs(U.fuse_(o), x), peaks)
        return cache[name]

    return get


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("name", list(MODULES))
def test_module_forward(module_case, name, half):
    p, x, (y64, y32, y16), peaks = module_case(name)
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
    assert any(w.startswith("AAttn.area") for w in whats)
    assert ("A2C2f.gamma" in whats) == (name == "A2C2f_gamma")
    assert d <= bound


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
@pytest.mark.parametrize("c1,c2,g,launches", [(16, 32, 2, 2), (64, 64, 4, 4), (24, 24, 2, 1)])
def test_grouped_conv(c1, c2, g, launches, dtype):
    """Conv(c1, c2, 3, 2, 1, g): one dense launch per group on channel slices, or (24 -> 24, g 2: 12 channels per
    group break the 16-byte vector rule) one block-diagonal dense launch; tolerance of test_gpu_ops' dense convs."""
    from ydbl.nn.modules import Conv
    from ydbl.utils.synthetic import trained_like_

    torch.manual_seed(c1 + c2 + g)
    m = trained_like_(Conv(c1, c2, 3, 2, 1, g).eval(), 1)
    x = torch.randn(2, c1, 16, 16)
    wf, bf = m.folded()
    ref = F.silu(F.conv2d(x.to(dtype).float(), wf.to(dtype).float(), bf, 2, 1, 1, g))
    got = m.cuda()(x.cuda().to(dtype))
    torch.cuda.synchronize()
    whats = [st.what for mp in m._fwd_plans.values() for st in mp.plan.steps]
    assert len(whats) == launches, whats
    tol = dict(rtol=2e-5, atol=2e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(got.float().cpu(), ref, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "half"])
def test_upsample_into_concat_slice(dtype):
    from ydbl.nn.modules import Upsample
    from ydbl.runtime import Plan

    x = torch.randn(2, 24, 5, 7, generator=torch.Generator().manual_seed(2)).to(dtype)
    plan = Plan(torch.device("cuda"), dtype)
    xv = plan.alloc(2, 5, 7, 24)
    xv.torch().copy_(x.permute(0, 2, 3, 1))
    buf = plan.alloc(2, 10, 14, 48)
    buf.torch().fill_(5.0)
    out = Upsample(None, 2, "nearest").emit(plan, xv, buf.cslice(16, 24))
    plan.run()
    torch.cuda.synchronize()
    assert torch.equal(out.nchw().cpu(), F.interpolate(x, scale_factor=2.0, mode="nearest"))
    rest = torch.cat([buf.torch()[..., :16], buf.torch()[..., 40:]], -1).cpu()
    assert torch.equal(rest, torch.full_like(rest, 5.0))
    assert torch.equal(Upsample(None, 2, "nearest")(x.cuda()).cpu(), F.interpolate(x, scale_factor=2.0, mode="nearest"))


# ----------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def pair():
    return U.build_pair("n", 3)


@pytest.fixture(scope="module")
def e2e_ref(pair):
    """(H, W) -> (x, the restatement's legs, their err_stats); computed once per shape."""
    from parity_util import err_stats, oracle_legs

    cache = {}

    def get(hw):
        if hw not in cache:
            x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[1]))
            ys, _ = oracle_legs(pair[1], x, legs=("fp64", "fp32", "fp16"))
            cache[hw] = (x, ys, {k: err_stats(ys[k], ys["fp64"]) for k in ("fp32", "fp16")})
        return cache[hw]

    return get


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("hw", [(128, 128), (96, 160)], ids=["128x128", "96x160"])
def test_e2e_yolov13n(pair, e2e_ref, hw, half):
    """96x160: a 6x10 map at stride 16, 15 tokens per chunk at area 4 (chunk boundaries mid-row)."""
    from parity_util import err_stats, fp16_rule, fp32_rule, gpu_pred

    p, _ = pair
    x, ys, st_ref = e2e_ref(hw)
    yg, _ = gpu_pred(p, x, half=half)
    assert yg.shape == ys["fp64"].shape
    st = err_stats(yg, ys["fp64"])
    if half:
        tb, tc = fp16_rule(st_ref["fp16"])
        got = (st["box_p999"], st["conf_p999"])
    else:
        tb, tc = fp32_rule(st_ref["fp32"])
        got = (st["box_max"], st["conf_max"])
    print(f"yolov13n {hw} {'half' if half else 'fp32'}: gpu {st} | restatement leg "
          f"{st_ref['fp16' if half else 'fp32']} | bound box {tb:.3g} score {tc:.3g}")
    assert got[0] <= tb and got[1] <= tc


def test_e2e_plan_routing(pair):
    """The plan runs the new launches: area attention at P4 and P5, per-group convs, three nearest upsamples."""
    p, _ = pair
    s = p.session(2, 96, 160, half=True, keep_pred=True, use_graph=False)
    whats = [st.what for st in s.plan.steps]
    assert whats.count("AAttn.area4") == 4 and whats.count("AAttn.area1") == 4  # 2 x (ABlock, ABlock) per A2C2f
    assert sum(w.startswith("Conv3x3.g") for w in whats) == 2 + 4
    assert whats.count("Upsample.nearest2") == 3


def test_e2e_streams2_bit_equal(pair):
    p, _ = pair
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


def test_predict_augment_returns_boxes(pair):
    p, _ = pair
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(9))
    res = p.predict(x, augment=True, conf=0.001, half=True)
    assert len(res) == 2
    for r in res:
        assert r.boxes.data.shape[1] == 6 and len(r.boxes) > 0 and torch.isfinite(r.boxes.data).all()


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_val_runs(pair, half):
    """val() on a tensor batch with made-up labels runs on the baseline model in both precisions (with init weights the
    class scores stay under val's conf 0.001, so there is nothing to match: the point is that the validation
    session -- multi-label NMS, matching, the report -- builds and runs on this model)."""
    p, _ = pair
    x = torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(10))
    boxes = torch.tensor([[10.0, 10.0, 60.0, 50.0], [30.0, 20.0, 120.0, 90.0], [5.0, 40.0, 70.0, 80.0]])
    batch = {"img": x, "bboxes": boxes, "cls": torch.tensor([0.0, 1.0, 2.0]), "batch_idx": torch.tensor([0, 0, 1])}
    p.val([batch], half=half)
    st = p.validator.stats
    assert len(torch.cat(st["target_cls"])) == 3
    assert torch.isfinite(torch.cat(st["conf"])).all()
