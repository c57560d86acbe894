"""embed() end to end on the MI355X: DBL-n, nc 3, the trained-like fixture, a seeded batch of 5 images 96 x 128 in
[0, 1].  Parity with the oracle's three precision legs (tests/embed_util.py), the pool kernel isolated inside the
plan, order / default / dtype, forward(), split sessions, the early exit, frame and path sources, stale weights.

Measured on the MI355X (embed [1, 9, 34], max over all elements, gpu deviation from fp64 / the oracle leg's own):
fp32 1.46e-4 / 1.14e-4 = 1.28, fp16 0.202 / 0.248 = 0.82 (the bound allows 2)."""

import numpy as np
import pytest
import torch

from embed_util import oracle_embed_legs, pool_bound

pytestmark = pytest.mark.gpu

B, H, W = 5, 96, 128
EMBED = [1, 9, 34]


@pytest.fixture(scope="module")
def pair(golden_dir):
    from parity_util import build_pair

    return build_pair("n", 3, golden_dir)


@pytest.fixture(scope="module")
def x():
    return torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(7))


@pytest.fixture(scope="module")
def legs(pair, x):
    """The oracle embedding [B, 400] in fp64 / fp32 / fp16 (as float64), computed once."""
    return oracle_embed_legs(pair[1], x, EMBED)


def fresh_model(golden_dir):
    """A product model of its own (tests that edit weights)."""
    from ydbl import YOLO
    from ydbl.utils.synthetic import load_trained

    torch.manual_seed(0)
    p = YOLO("yolov13n_DBL.yaml", nc=3)
    load_trained(p.model, golden_dir / "trained_yolov13n_DBL_nc3.npz")
    return p


def bounds(legs):
    """(fp32, fp16) element bounds: parity_util.fp32_rule / fp16_rule's form on the embedding."""
    return (2 * (legs["fp32"] - legs["fp64"]).abs().max().item() + 1e-6,
            2 * (legs["fp16"] - legs["fp64"]).abs().max().item() + 1e-3)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_parity_with_the_oracle_legs(pair, x, legs, half):
    p, _ = pair
    got = torch.stack(p.predict(x.cuda(), embed=EMBED, half=half))
    assert got.shape == (B, 16 + 128 + 256) and got.dtype == (torch.float16 if half else torch.float32)
    assert got.device.type == "cuda"
    leg = "fp16" if half else "fp32"
    bound = bounds(legs)[int(half)]
    dev = (got.cpu().double() - legs["fp64"]).abs().max().item()
    odev = (legs[leg] - legs["fp64"]).abs().max().item()
    print(f"embed parity {leg}: gpu_dev {dev:.4g} oracle_dev {odev:.4g} ratio {dev / odev:.3f} bound {bound:.4g}")
    assert dev <= bound, (dev, odev)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_pool_kernel_isolated_inside_the_plan(pair, x, half):
    """The pool's own input, read back from the plan, averaged in fp64: a pooling bug shows here, upstream conv
    deviation does not."""
    p, _ = pair
    s = p.session(B, H, W, half=half, embed=EMBED, streams=1)
    out = s(x.cuda()).clone()
    torch.cuda.synchronize()
    v = s.compiled.embed_views[34].torch().cpu()  # nothing runs behind layer 34: the view is as the pool read it
    assert v.shape == (B, 3, 4, 256)
    err = (out[:, -256:].cpu().double() - v.double().mean((1, 2))).abs()
    assert (err <= pool_bound(v, half)).all(), (err / pool_bound(v, half)).max().item()


def test_order_default_and_dtype(pair, x):
    p, _ = pair
    xc = x.cuda()
    a = torch.stack(p.predict(xc, embed=[34, 1, 9]))
    b = torch.stack(p.predict(xc, embed=[1, 9, 34, 9]))
    assert torch.equal(a, b)
    d = p.embed(xc)
    e = p.predict(xc, embed=[34])
    assert isinstance(d, list) and len(d) == B and all(t.shape == (256,) and t.dtype == torch.float32 for t in d)
    assert all(torch.equal(u, v) for u, v in zip(d, e))
    assert torch.equal(torch.stack(d), a[:, -256:])  # the same layer-34 segment, whatever else is pooled
    h = p.embed(xc, half=True)
    assert all(t.shape == (256,) and t.dtype == torch.float16 for t in h)
    g = p.embed(xc, stream=True)
    assert not isinstance(g, list) and all(torch.equal(u, v) for u, v in zip(g, d))
    # the result is the caller's: a later call does not rewrite it
    keep = [t.clone() for t in d]
    p.embed(torch.rand_like(xc))
    assert all(torch.equal(u, v) for u, v in zip(d, keep))
    # a host tensor takes the same route; a 0..255 batch is multiplied by fp32(1/255) on the way in (LoadTensor's rule)
    assert torch.equal(torch.stack(p.embed(x)), torch.stack(d))
    x255 = xc * 255.0
    scaled = x255 * torch.tensor(1.0 / 255.0, dtype=torch.float32, device="cuda")
    assert x255.max() > 2 and scaled.max() <= 1.0
    assert torch.equal(torch.stack(p.embed(x255)), torch.stack(p.embed(scaled)))


def test_sessions_are_shared_across_detection_arguments(pair):
    p, _ = pair
    a = p.session(B, H, W, embed=[34], conf=0.5)
    assert p.session(B, H, W, embed=(34, 34), conf=0.25, iou=0.3, max_det=10) is a
    assert p.session(B, H, W, embed=[9]) is not a
    assert type(a).__name__ == "EmbedSession" and a.out.shape == (B, 256)


def test_forward_returns_the_unbound_rows(pair, x):
    from ydbl.engine.session import default_streams

    p, _ = pair
    xc = x.cuda()
    y = p.model(xc, embed=[9])
    assert isinstance(y, tuple) and len(y) == B and all(t.shape == (128,) and t.dtype == torch.float32 for t in y)
    ref = p.predict(xc, embed=[9], streams=default_streams(B))
    assert all(torch.equal(u, v) for u, v in zip(y, ref))
    yh = p.model(xc.half(), embed=[9])
    assert all(t.dtype == torch.float16 for t in yh)
    assert torch.equal(torch.stack(yh), torch.stack(p.predict(xc, embed=[9], half=True)))


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_split_session_against_one_plan(pair, x, legs, half):
    p, _ = pair
    s1 = p.session(B, H, W, half=half, embed=(34,), streams=1)
    s2 = p.session(B, H, W, half=half, embed=(34,), streams=2)
    assert [c.batch for c in s2.children] == [3, 2] and len(s1.children) == 0
    o1, o2 = s1(x.cuda()).clone(), s2(x.cuda()).clone()
    o2b = s2(x.cuda()).clone()  # the replayed graph
    torch.cuda.synchronize()
    assert torch.equal(o2, o2b)
    bound = bounds(legs)[int(half)]
    y64 = legs["fp64"][:, -256:]
    for o in (o1, o2):
        assert (o.cpu().double() - y64).abs().max().item() <= bound
    assert (o1.double() - o2.double()).abs().max().item() <= 2 * bound


def test_early_exit_is_real(pair, x, golden_dir):
    p, _ = pair
    e = p.session(B, H, W, embed=[34], streams=1)
    d = p.session(B, H, W, streams=1)
    assert len(e.plan.steps) < len(d.plan.steps)
    assert not any(st.what.startswith(("Detect", "NMS")) for st in e.plan.steps)
    q = fresh_model(golden_dir)
    xc = x.cuda()
    before = torch.stack(q.embed(xc))
    with torch.no_grad():
        for t in q.model.model[-1].parameters():
            t.zero_()
    q.reset_sessions()
    after = torch.stack(q.embed(xc))
    assert torch.equal(before, after)
    assert torch.equal(before, torch.stack(p.embed(xc)))


def test_frame_source_goes_through_letterbox(pair):
    from ydbl.engine.preprocess import letterbox_batch

    p, _ = pair
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (60, 90, 3), dtype=np.uint8), rng.integers(0, 256, (100, 80, 3), dtype=np.uint8)]
    im = letterbox_batch(frames, (128, 128), stride=int(p.model.stride.max()), device="cuda")
    assert im.shape == (2, 3, 128, 128)
    a = p.predict(frames, embed=[34], imgsz=128)
    b = p.predict(im, embed=[34])
    assert len(a) == 2 and all(t.shape == (256,) for t in a)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    one = p.embed(frames[0], imgsz=128)  # a single frame is a batch of one (minimum-rectangle letterbox)
    assert len(one) == 1 and one[0].shape == (256,)


def test_path_source_in_batches(pair, tmp_path):
    from PIL import Image

    from ydbl.engine.dataset import load_bgr

    p, _ = pair
    rng = np.random.default_rng(5)
    files = []
    for i, (h, w) in enumerate([(40, 64), (64, 48), (50, 50)]):
        f = tmp_path / f"im{i}.png"
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(f)
        files.append(f)
    got = p.predict(str(tmp_path), embed=[34], imgsz=64, batch=2)
    assert len(got) == 3 and all(t.shape == (256,) for t in got)
    first = p.predict([load_bgr(f) for f in files[:2]], embed=[34], imgsz=64)
    last = p.predict([load_bgr(files[2])], embed=[34], imgsz=64)
    assert all(torch.equal(u, v) for u, v in zip(got, list(first) + list(last)))
    gen = p.predict(str(tmp_path), embed=[34], imgsz=64, batch=2, stream=True)
    assert not isinstance(gen, list) and all(torch.equal(u, v) for u, v in zip(gen, got))


def test_stale_weights_rebuild_the_session(x, golden_dir):
    q = fresh_model(golden_dir)
    xc = x.cuda()
    before = torch.stack(q.embed(xc))
    assert torch.equal(torch.stack(q.model(xc, embed=[34])), before)  # (forward()'s own session, compiled now)
    conv = next(m for m in q.model.model[2].modules() if isinstance(m, torch.nn.Conv2d))
    with torch.no_grad():
        conv.weight.mul_(1.25)
    after = torch.stack(q.embed(xc))
    assert not torch.equal(before, after)
    r = fresh_model(golden_dir)
    r.model.load_state_dict(q.model.state_dict())
    assert torch.equal(after, torch.stack(r.embed(xc)))
    # forward() notices too
    with torch.no_grad():
        conv.weight.mul_(0.8)
    y = torch.stack(q.model(xc, embed=[34]))
    r.model.load_state_dict(q.model.state_dict())
    assert torch.equal(y, torch.stack(r.embed(xc)))
