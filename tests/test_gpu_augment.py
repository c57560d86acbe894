"""Test-time augmentation (augment=True) on the MI355X: the scale_img kernel, the merged prediction and its NMS,
parity with the oracle's restated pipeline (tests/augment_util.py), graph replay, predict / forward / val.

DBL-n, nc 3, the trained-like fixture; (160, 224) inputs give three different pass shapes -- (160, 224),
(160, 192), (128, 160) -- and a merged anchor axis of 700 + 630 + 100."""

import numpy as np
import pytest
import torch

from augment_util import PAD_VALUE, blob_batch, merge_passes, oracle_augment, pass_sizes, scale_img_cpu

pytestmark = pytest.mark.gpu

H, W = 160, 224


@pytest.fixture(scope="module")
def pair(golden_dir):
    from parity_util import build_pair

    return build_pair("n", 3, golden_dir)


@pytest.mark.parametrize("shape", [(2, 3, 160, 224), (2, 3, 96, 64)])
@pytest.mark.parametrize("ratio", [0.83, 0.67])
@pytest.mark.parametrize("flip", [False, True])
def test_scale_img_kernel(shape, ratio, flip):
    """ydbl_scale_img vs torch-CPU scale_img in fp32 (t32) and fp64 (t64): exact shape, pad region exactly fp32 0.447,
    and on the resized region no farther from the fp64 answer than twice torch's own fp32 error e (+1e-6), and
    within e + 1e-6 of torch's fp32 result.  A wrong neighbour or a missed flip is an error of order 0.1."""
    from ydbl.engine.preprocess import scale_img

    x = torch.rand(shape, generator=torch.Generator().manual_seed(shape[2] + int(100 * ratio) + flip))
    t32 = scale_img_cpu(x, ratio, flip)
    t64 = scale_img_cpu(x.double(), ratio, flip)
    got = scale_img(x.cuda(), ratio, flip=flip)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.float32
    got = got.cpu()
    (sh, sw), (hp, wp) = pass_sizes(shape[2], shape[3], ratio)
    assert tuple(got.shape) == tuple(t32.shape) == (shape[0], shape[1], hp, wp)
    pad = torch.ones(hp, wp, dtype=torch.bool)
    pad[:sh, :sw] = False
    assert pad.any() and torch.equal(got[:, :, pad], torch.full_like(got[:, :, pad], PAD_VALUE))
    assert torch.equal(t32[:, :, pad], got[:, :, pad])
    r32, r64, rg = t32[:, :, :sh, :sw], t64[:, :, :sh, :sw], got[:, :, :sh, :sw]
    e = (r32.double() - r64).abs().max().item()
    d64 = (rg.double() - r64).abs().max().item()
    d32 = (rg - r32).abs().max().item()
    print(f"scale_img {shape} r={ratio} flip={flip}: torch fp32 error e={e:.3g}, |gpu-t64|={d64:.3g}, |gpu-t32|={d32:.3g}")
    assert d64 <= 2 * e + 1e-6
    assert d32 <= e + 1e-6


def test_scale_img_unaligned_width_and_identity():
    """A padded width that is no multiple of 4 takes the scalar-store path; ratio 1.0 returns the (mirrored) input."""
    from ydbl.engine.preprocess import scale_img

    x = torch.rand(1, 3, 50, 70, generator=torch.Generator().manual_seed(3))
    got = scale_img(x.cuda(), 0.83, flip=True, gs=7).cpu()
    want = scale_img_cpu(x, 0.83, True, gs=7)
    w64 = scale_img_cpu(x.double(), 0.83, True, gs=7)
    assert got.shape == want.shape and got.shape[3] % 4 != 0
    e = (want.double() - w64).abs().max().item()  # the same bounds as test_scale_img_kernel
    assert (got.double() - w64).abs().max().item() <= 2 * e + 1e-6 and (got - want).abs().max().item() <= e + 1e-6
    assert torch.equal(got[:, :, :, int(70 * 0.83):], want[:, :, :, int(70 * 0.83):])
    xc = x.cuda()
    assert scale_img(xc, 1.0) is xc and torch.equal(scale_img(xc, 1.0, flip=True).cpu(), x.flip(3))
    with pytest.raises(RuntimeError):
        scale_img(x, 0.83)


def _plain_pred(p, x, **kw):
    b, _, h, w = x.shape
    s = p.session(b, h, w, half=False, conf=0.05, iou=0.7, keep_pred=True, use_graph=False, **kw)
    s(x)
    torch.cuda.synchronize()
    return s.pred.cpu()


def test_merged_pred_bit_exact_vs_plain_sessions(pair):
    """The augment session's merged pred == de-scale / de-flip / tail clip / cat, done with torch-CPU ops, of three
    plain sessions run on x, scale_img(x, .83, flip) and scale_img(x, .67): pins the division rule, the anchor
    windows, pos_base and the y_ref stride, with no tolerance."""
    from ydbl.engine.preprocess import scale_img

    p, _ = pair
    x = blob_batch(2, H, W, seed=1234).cuda()
    s = p.session(2, H, W, half=False, conf=0.05, iou=0.7, keep_pred=True, use_graph=False, augment=True)
    s(x)
    torch.cuda.synchronize()
    got = s.pred.cpu()
    ys = [_plain_pred(p, x), _plain_pred(p, scale_img(x, 0.83, flip=True)), _plain_pred(p, scale_img(x, 0.67))]
    assert [y.shape[-1] for y in ys] == [735, 630, 420]
    want = merge_passes(ys, W)
    assert got.shape == want.shape == (2, 7, 1430)
    assert torch.equal(got, want)


@pytest.mark.parametrize("batch,streams", [(2, 1), (4, 2)])
def test_merged_nms_bit_exact(pair, batch, streams):
    """GPU NMS over the three passes' union == the oracle's NMS on the session's own merged pred (then clip_boxes),
    array for array; batch 4 runs two sub-batch branches of one graph."""
    from oracle.ops import clip_boxes, non_max_suppression

    p, _ = pair
    x = blob_batch(batch, H, W, seed=77).cuda()
    for conf, multi in ((0.05, False), (0.001, True)):
        s = p.session(batch, H, W, half=False, conf=conf, iou=0.7, multi_label=multi, keep_pred=True, augment=True,
                      streams=streams)
        assert len(s.children) == (streams if streams > 1 else 0)
        s(x)
        ref = non_max_suppression(s.pred.cpu(), conf, 0.7, multi_label=multi)
        got = s.results()
        assert sum(len(g) for g in got) > 0
        for r, g in zip(ref, got):
            clip_boxes(r[:, :4], (H, W))
            assert np.array_equal(g.numpy(), r.numpy())


def test_augment_parity_with_oracle(pair):
    """The merged pred vs the restated pipeline run with the oracle in fp64, under parity_util.fp32_rule of the
    oracle's fp32 leg (as test_model_fp32_parity), at 160^2.
    Measured on the MI355X: gpu |dbox| 4.32e-4 px, |dconf| 2.25e-6 against the oracle fp32 leg's 5.32e-4 px,
    1.83e-6; 161 matched detections, 0 borderline, box dev 9.16e-5 px, conf dev 2.25e-6."""
    from parity_util import class_agreement, detections, err_stats, fp32_rule, match_detections

    p, o = pair
    x = blob_batch(2, 160, 160, seed=1234)
    ys = oracle_augment(o, x, ("fp64", "fp32"))
    y64 = ys["fp64"]
    s = p.session(2, 160, 160, half=False, conf=0.05, iou=0.7, keep_pred=True, use_graph=False, augment=True)
    s(x.cuda())
    torch.cuda.synchronize()
    y = s.pred.cpu()
    assert y.shape == y64.shape
    o32 = err_stats(ys["fp32"], y64)
    st = err_stats(y, y64)
    tb, tc = fp32_rule(o32)
    print(f"augment parity 160^2: gpu |dbox| {st['box_max']:.3g} px, |dconf| {st['conf_max']:.3g}; "
          f"oracle fp32 {o32['box_max']:.3g} px, {o32['conf_max']:.3g}")
    assert st["box_max"] <= tb and st["conf_max"] <= tc
    checked, bad = class_agreement(y, y64, tc)
    assert bad == 0 and checked > 0
    ref = detections(y64, 0.05, 0.7, (160, 160))
    m = match_detections(ref, s.results(), y64, 0.05, 0.7, tb, tc)
    print(f"augment parity 160^2: {m['pairs']} matched detections, {m['borderline']} borderline, "
          f"box dev {m['box_dev']:.3g} px, conf dev {m['conf_dev']:.3g}")
    assert m["pairs"] > 0 and not m["mismatches"], m["mismatches"][:5]


def test_augment_graph_replay_equals_eager(pair):
    """One captured graph replayed on two different batches == the eager session on each: the candidate counters
    are zeroed by pass 0 of every replay and appended to by passes 1 and 2, so nothing accumulates."""
    p, _ = pair
    xa, xb = blob_batch(2, H, W, seed=9).cuda(), blob_batch(2, H, W, seed=10).cuda()
    kw = dict(half=True, conf=0.05, keep_pred=True, augment=True)
    s_eager = p.session(2, H, W, use_graph=False, **kw)
    s_graph = p.session(2, H, W, use_graph=True, **kw)
    assert s_eager is not s_graph
    seen = []
    for x in (xa, xb, xa):
        d0, c0 = (t.clone() for t in s_eager(x))
        p0, n0 = s_eager.pred.clone(), s_eager.cand_count.clone()
        d1, c1 = s_graph(x)
        torch.cuda.synchronize()
        assert torch.equal(c0, c1) and torch.equal(d0, d1) and torch.equal(p0, s_graph.pred)
        assert torch.equal(n0, s_graph.cand_count)
        seen.append((d1.clone(), c1.clone()))
    assert int(seen[0][1].sum()) > 0 and not torch.equal(seen[0][0], seen[1][0])
    assert torch.equal(seen[0][0], seen[2][0]) and torch.equal(seen[0][1], seen[2][1])


def test_augment_public_api(pair):
    """predict(x, augment=True) returns the augment session's boxes and differs from plain predict; the model's
    forward(augment=True) returns (merged y, None); half + augment agrees with fp32 + augment in detection counts
    (the rule of test_fp16_detections_agree)."""
    p, _ = pair
    x = blob_batch(2, H, W, seed=11)
    s = p.session(2, H, W, half=False, conf=0.05, iou=0.7, keep_pred=True, use_graph=False, augment=True)
    s(x.cuda())
    want = s.results()
    pred = s.pred.clone()
    res = p.predict(x, conf=0.05, augment=True)
    plain = p.predict(x, conf=0.05)
    assert len(res) == 2
    for r, w in zip(res, want):
        assert torch.equal(r.boxes.data.cpu(), w)
    assert any(a.boxes.data.shape != b.boxes.data.shape or not torch.equal(a.boxes.data, b.boxes.data)
               for a, b in zip(res, plain))
    again = p.predict(x, conf=0.05)  # the plain path is what it was: its own session, untouched by the augment one
    for a, b in zip(plain, again):
        assert torch.equal(a.boxes.data, b.boxes.data)
    y, feats = p.model(x.cuda(), augment=True)
    assert feats is None and torch.equal(y, pred)
    y_plain, f_plain = p.model(x.cuda())
    assert y_plain.shape[-1] == 735 and len(f_plain) == 3
    with pytest.raises(NotImplementedError):
        p.model(x.cuda(), profile=True)
    half = p.predict(x, conf=0.05, half=True, augment=True)
    for r, g in zip(want, half):
        if min(len(r), len(g.boxes.data)):
            assert abs(len(r) - len(g.boxes.data)) <= max(2, len(r) // 5)


def test_augment_val(pair):
    """val([batch], augment=True): the validator's stats == those built from the augment session's detections
    (conf 0.001, multi_label) with match_batch."""
    from ydbl.engine.validator import match_batch
    from ydbl.utils.metrics import IOUV

    p, _ = pair
    x = blob_batch(4, 160, 160, seed=21)
    # pseudo labels: the plain path's confident boxes
    labels = p.predict(x, conf=0.25)
    boxes = torch.cat([r.boxes.data[:, :4].cpu() for r in labels])
    cls = torch.cat([r.boxes.data[:, 5].cpu() for r in labels])
    bidx = torch.cat([torch.full((len(r.boxes.data),), i) for i, r in enumerate(labels)])
    assert len(boxes) > 0
    batch = {"img": x, "bboxes": boxes, "cls": cls, "batch_idx": bidx}
    p.val([batch], augment=True)
    st = p.validator.stats
    s = p.session(4, 160, 160, half=False, conf=0.001, iou=0.7, multi_label=True, augment=True)
    assert type(s).__name__ == "AugmentSession"
    det, cnt = s(x.cuda())
    tp = match_batch(det, cnt, boxes, cls, bidx, IOUV).cpu()
    det, cnt = det.cpu(), cnt.cpu().tolist()
    assert sum(cnt) > 0
    assert torch.equal(torch.cat(st["tp"]), torch.cat([tp[i, : cnt[i]] for i in range(4)]))
    assert torch.equal(torch.cat(st["conf"]), torch.cat([det[i, : cnt[i], 4] for i in range(4)]))
    assert torch.equal(torch.cat(st["pred_cls"]), torch.cat([det[i, : cnt[i], 5] for i in range(4)]))
    # and it is not the plain validation: the un-augmented run keeps fewer or other detections
    p.val([batch])
    assert not (len(torch.cat(p.validator.stats["conf"])) == sum(cnt)
                and torch.equal(torch.cat(p.validator.stats["conf"]), torch.cat(st["conf"])))
