"""ydbl_hg_fused_pair: two independent AdaHGConv calls of one shape in one set of five launches (blockIdx.z picks
the call).  Kernel level through the C ABI: the buffer after the pair call equals, bit for bit, the buffer after
ydbl_hg_fused(d0) then ydbl_hg_fused(d1) -- the per-image arithmetic is the same, so there is no tolerance -- and the
descriptors that must not pair (other batch, other edge count, a chained input) fall back to the two calls.  Module
level: HyperACE's two C3AH branches share one "AdaHG.fused2" step, and YDBL_NO_HG_PAIR=1 restores the two
"AdaHG.fused" steps with the same output bits.  Session level: det / count / cand_count of DBL-n unchanged."""

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _plan(dtype):
    from ydbl.runtime import Plan

    return Plan(torch.device(DEV), dtype)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _hg(dim, edges, seed):
    from ydbl.nn import modules as M

    torch.manual_seed(seed)
    return M.AdaHGConv(dim, edges, dim // 16).eval()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _branch_buffer(plan, b, h, w, dim, seed):
    """[B, h, w, 6 D] laid out as HyperACE._emit_branches lays out bb: [m2 | . | x2 | x1 | . | m1]."""
    bb = plan.alloc(b, h, w, 6 * dim)
    g = torch.Generator().manual_seed(seed)
    bb.base.copy_(torch.randn(bb.base.numel(), generator=g).to(plan.dtype))
    return bb


def _check_pair_equals_singles(bufs, d0, d1, wss):
    """Run d0 then d1 as single calls, then the pair call twice (from the same initial buffers, the workspaces
    filled with 0xff first: nothing in them may be read before it is written); all three results equal."""
    from ydbl import _lib

    lib = _lib.lib
    init = [t.clone() for t in bufs]
    assert lib.ydbl_hg_fused(d0, _stream()) == 0 and lib.ydbl_hg_fused(d1, _stream()) == 0
    torch.cuda.synchronize()
    want = [t.clone() for t in bufs]
    assert any(not torch.equal(_bits(a), _bits(b)) for a, b in zip(want, init))  # the calls wrote something
    for ws in wss:
        ws.fill_(0xFF)
    for _ in range(2):
        for t, t0 in zip(bufs, init):
            t.copy_(t0)
        assert lib.ydbl_hg_fused_pair(d0, d1, _stream()) == 0
        torch.cuda.synchronize()
        for t, tw in zip(bufs, want):
            assert torch.equal(_bits(t), _bits(tw))
            assert not torch.isnan(t.float()).any()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("h,w", [(5, 7), (9, 9), (16, 8)])  # 35 / 81 / 128 tokens: partial, full + ragged, two full
@pytest.mark.parametrize("dim,edges", [(64, 4), (64, 8), (128, 4), (128, 8)])
def test_pair_equals_two_single_calls(dtype, b, h, w, dim, edges):
    plan = _plan(dtype)
    bb = _branch_buffer(plan, b, h, w, dim, seed=dim + edges + h)
    m2, m1 = _hg(dim, edges, 11), _hg(dim, edges, 12)
    f2 = m2.fused_desc(plan, bb.cslice(2 * dim, dim), bb.cslice(0, dim))
    f1 = m1.fused_desc(plan, bb.cslice(3 * dim, dim), bb.cslice(5 * dim, dim))
    assert f2 is not None and f1 is not None
    assert bb.cs == 6 * dim > dim  # the pixel stride is larger than the channel count
    _check_pair_equals_singles([bb.base], f2[0], f1[0], [f2[1][3], f1[1][3]])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", ["batch", "edges", "chained"])
def test_fallback_runs_the_two_calls_in_order(dtype, case):
    dim, h, w = 64, 9, 9
    plan = _plan(dtype)
    bb = _branch_buffer(plan, 2, h, w, dim, seed=3)
    bufs = [bb.base]
    m2 = _hg(dim, 4, 21)
    f2 = m2.fused_desc(plan, bb.cslice(2 * dim, dim), bb.cslice(0, dim))
    if case == "batch":  # d1 works on three images of another buffer
        b3 = _branch_buffer(plan, 3, h, w, dim, seed=4)
        bufs.append(b3.base)
        f1 = _hg(dim, 4, 22).fused_desc(plan, b3.cslice(3 * dim, dim), b3.cslice(5 * dim, dim))
    elif case == "edges":
        f1 = _hg(dim, 8, 22).fused_desc(plan, bb.cslice(3 * dim, dim), bb.cslice(5 * dim, dim))
    else:  # d1 reads what d0 writes: only the calls in order give d1 its input
        f1 = _hg(dim, 4, 22).fused_desc(plan, bb.cslice(0, dim), bb.cslice(5 * dim, dim))
    _check_pair_equals_singles(bufs, f2[0], f1[0], [f2[1][3], f1[1][3]])


def test_null_descriptor_is_einval():
    from ydbl import _lib

    plan = _plan(torch.float16)
    bb = _branch_buffer(plan, 1, 5, 7, 64, seed=1)
    d = _hg(64, 4, 1).fused_desc(plan, bb.cslice(128, 64), bb.cslice(0, 64))[0]
    before = bb.base.clone()
    lib = _lib.lib
    assert lib.ydbl_hg_fused_pair(None, d, _stream()) == 1 and "null descriptor" in lib.ydbl_last_error().decode()
    assert lib.ydbl_hg_fused_pair(d, None, _stream()) == 1
    assert lib.ydbl_hg_fused_pair(None, None, _stream()) == 1
    torch.cuda.synchronize()
    assert torch.equal(_bits(bb.base), _bits(before))


# ---------------------------------------------------------------------------------------------- module level
def _hyperace_plan(mod, xs, dtype):
    plan = _plan(dtype)
    views = []
    for x in xs:
        v = plan.alloc(*[x.shape[i] for i in (0, 2, 3, 1)])
        v.torch().copy_(x.permute(0, 2, 3, 1).to(dtype))
        views.append(v)
    out = mod.emit(plan, views)
    plan.run()
    torch.cuda.synchronize()
    return [st.what for st in plan.steps], out.torch().clone()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("c", [128, 64])
def test_hyperace_pairs_its_branches(dtype, c, monkeypatch):
    """c = 128: test_hyperace's module at twice the width, so the branches run at D = 64, the narrowest the one-call
    kernels take.  c = 64 is test_hyperace's own module: its branches run at D = 32, which has no one-call kernel
    (ydbl_hg_fused_workspace = -1, before this pairing and after), so both plans take the staged route and there is
    nothing to pair; the outputs still have to agree."""
    from ydbl.nn import modules as M

    torch.manual_seed(6)
    mod = M.HyperACE(c, c, 1, 4, True, True, 0.5, 1, "both", True).eval()
    xs = [torch.randn(2, c, 16, 16), torch.randn(2, c, 8, 8), torch.randn(2, 2 * c, 4, 4)]
    whats, out = _hyperace_plan(mod, xs, dtype)
    monkeypatch.setenv("YDBL_NO_HG_PAIR", "1")
    whats0, out0 = _hyperace_plan(mod, xs, dtype)
    assert "C3AHx2.cv1|cv2" in whats and "C3AHx2.cv1|cv2" in whats0 and "AdaHG.fused2" not in whats0
    if c == 128:
        assert whats.count("AdaHG.fused2") == 1 and "AdaHG.fused" not in whats
        k = whats.index("AdaHG.fused2")
        assert whats[k - 1] == "C3AHx2.cv1|cv2" and whats[k + 1 : k + 3] == ["Conv1x1", "Conv1x1"]
        assert whats0.count("AdaHG.fused") == 2
    else:
        assert whats == whats0 and whats.count("AdaHG.propagate") == 2 and "AdaHG.fused" not in whats
    assert torch.equal(_bits(out), _bits(out0))
    assert out.float().abs().max() > 0 and torch.isfinite(out.float()).all()
    # the staged route never pairs, with or without the switch
    monkeypatch.setenv("YDBL_HG_UNFUSED", "1")
    for no_pair in ("1", None):
        if no_pair is None:
            monkeypatch.delenv("YDBL_NO_HG_PAIR")
        w, _ = _hyperace_plan(mod, xs, dtype)
        assert "AdaHG.fused2" not in w and "AdaHG.fused" not in w and w.count("AdaHG.propagate") == 2


# ---------------------------------------------------------------------------------------------- session level
@pytest.fixture(scope="module")
def dbl_n(golden_dir):
    from ydbl import YOLO
    from ydbl.utils.synthetic import load_trained

    torch.manual_seed(0)
    p = YOLO("yolov13n_DBL.yaml", nc=3)
    load_trained(p.model, golden_dir / "trained_yolov13n_DBL_nc3.npz")
    return p


def _session_outputs(model, x, streams):
    s = model.session(3, 96, 96, half=True, conf=0.25, iou=0.7, streams=streams)
    d, c = s(x)
    torch.cuda.synchronize()
    whats = [st.what for p in s.plans for st in p.steps]
    return whats, d.clone(), c.clone(), s.cand_count.clone()


@pytest.mark.parametrize("streams", [1, 2])
def test_session_outputs_unchanged(dbl_n, streams, monkeypatch):
    from ydbl.utils.synthetic import blob_images

    x = blob_images(3, 96, seed=5).cuda()
    whats, d, c, n = _session_outputs(dbl_n, x, streams)
    assert "AdaHG.fused2" in whats and "AdaHG.fused" not in whats
    monkeypatch.setenv("YDBL_NO_HG_PAIR", "1")
    whats0, d0, c0, n0 = _session_outputs(dbl_n, x, streams)
    assert "AdaHG.fused2" not in whats0 and whats0.count("AdaHG.fused") == 2 * whats.count("AdaHG.fused2")
    assert torch.equal(n, n0) and torch.equal(c, c0)
    assert d.dtype == d0.dtype == torch.float32 and torch.equal(_bits(d), _bits(d0))
    assert int(c0.sum()) > 0
