"""ydbl_detect_topk and ydbl_detect_decode_e2e on the MI355X.

The selection is checked exactly (torch.equal) on synthetic candidate lists against the pinned-order restatement of
tests/yolov10_util.py (a plain sort by (score descending, cand_idx ascending)), in both schedules (per_image 1: one
workgroup per image; 0: histogram + compaction ahead of it).  The lists are written in a random order with distinct
cand_idx, so neither the order of the list nor of the atomics may show in the result.  The decode is checked against
the restated v10Detect._inference (dist2bbox(xywh=False) * stride in fp32) on the same logits."""

import ctypes as C

import pytest
import torch

import yolov10_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"


def make_list(n, cap, nc, seed, scores=None):
    """One image's candidates in list order: (box [n,4], score [n], cls [n], idx [n]); idx distinct in [0, cap)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(cap, generator=g)[:n].int()
    sc = torch.rand(n, generator=g) * 0.98 + 0.01 if scores is None else scores
    xy = torch.rand(n, 2, generator=g) * 200 - 20
    wh = torch.rand(n, 2, generator=g) * 100
    return torch.cat([xy, xy + wh], 1), sc.float(), (idx % nc).int(), idx


def run_topk(lists, cap, k_head, max_det, per_image, classes=None, clip=(0.0, 0.0), record_pad=0):
    """The kernel on a batch of lists -> (det [B, max_det, 6], count [B], the whole output record buffer) on the
    host.  Slots past an image's count hold NaN scores and out-of-range indices: they must never be read."""
    from ydbl import _lib

    B = len(lists)
    cb = torch.full((B, cap, 4), float("nan"))
    cs = torch.full((B, cap), float("nan"))
    cc = torch.full((B, cap), -7, dtype=torch.int32)
    ci = torch.full((B, cap), -1, dtype=torch.int32)
    cn = torch.zeros(B, dtype=torch.int32)
    for b, (box, sc, cls, idx) in enumerate(lists):
        n = len(sc)
        cb[b, :n], cs[b, :n], cc[b, :n], ci[b, :n], cn[b] = box, sc, cls, idx, n
    cb, cs, cc, ci, cn = (t.to(DEV) for t in (cb, cs, cc, ci, cn))
    width = max_det * 6 + (1 + record_pad if record_pad else 0)
    rec = torch.full((B, width), -5.0, device=DEV)
    if record_pad:  # one record per image [det | count | pad], as the batch-sharded predictor's
        out_ptr, cnt_ptr, ostride, cstride = rec.data_ptr(), rec.data_ptr() + max_det * 6 * 4, width, width
        count = None
    else:
        count = torch.full((B,), -9, dtype=torch.int32, device=DEV)
        out_ptr, cnt_ptr, ostride, cstride = rec.data_ptr(), count.data_ptr(), 0, 0
    ct = torch.tensor(list(classes), dtype=torch.int32, device=DEV) if classes is not None else None
    nws = int(_lib.lib.ydbl_detect_topk_workspace(B, cap))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    d = _lib.TopkDesc(cb.data_ptr(), cs.data_ptr(), cc.data_ptr(), ci.data_ptr(), cn.data_ptr(), B, cap, k_head,
                      max_det, ct.data_ptr() if ct is not None else None, len(ct) if ct is not None else 0,
                      float(clip[1]), float(clip[0]), out_ptr, cnt_ptr, ostride, cstride, ws.data_ptr(), nws,
                      int(per_image))
    _lib.check(_lib.lib.ydbl_detect_topk(C.byref(d), None), "ydbl_detect_topk")
    torch.cuda.synchronize()
    rec = rec.cpu()
    det = rec[:, : max_det * 6].reshape(B, max_det, 6)
    cnt = rec[:, max_det * 6].contiguous().view(torch.int32) if record_pad else count.cpu()
    return det, cnt, rec


def check(lists, det, cnt, k_head, max_det, classes=None, clip=None):
    for b, (box, sc, cls, idx) in enumerate(lists):
        want = U.select_candidates(box, sc, cls, idx, k_head, max_det, classes, clip)
        n = int(cnt[b])
        assert n == len(want), (b, n, len(want))
        assert torch.equal(det[b, :n], want), b
        assert not det[b, n:].any(), b  # rows past the count are zero


MODES = pytest.mark.parametrize("per_image", [1, 0], ids=["per_image", "split"])
K = 300
COUNTS = [0, 1, K - 1, K, K + 1, 1023, 1024, 1025, 26880, 131075]  # one batch, very different counts mixed


@pytest.fixture(scope="module")
def big_batch():
    """The count ladder as ONE batch (cap 131075: past any 16-bit counter), nc 80; built once, left unchanged."""
    cap = COUNTS[-1]
    return cap, [make_list(n, cap, 80, 100 + i) for i, n in enumerate(COUNTS)]


@MODES
def test_count_ladder_mixed_batch(big_batch, per_image):
    cap, lists = big_batch
    det, cnt, _ = run_topk(lists, cap, K, K, per_image)
    assert cnt.tolist() == [min(n, K) for n in COUNTS]
    check(lists, det, cnt, K, K)
    det2, cnt2, _ = run_topk(lists, cap, K, K, per_image)  # two runs bit-identical
    assert torch.equal(det.view(torch.int32), det2.view(torch.int32)) and torch.equal(cnt, cnt2)


def test_schedules_agree(big_batch):
    cap, lists = big_batch
    a, b = run_topk(lists, cap, K, K, 1), run_topk(lists, cap, K, K, 0)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


@MODES
@pytest.mark.parametrize("max_det", [1, 7, 300])
def test_max_det(per_image, max_det):
    cap = 2000
    lists = [make_list(n, cap, 3, 7 * max_det + n) for n in (0, 1, 6, 7, 8, 299, 300, 301, 1025)]
    det, cnt, _ = run_topk(lists, cap, 300, max_det, per_image)
    check(lists, det, cnt, 300, max_det)


@MODES
def test_k_head_below_max_det(per_image):
    """A = 21 anchors, nc 3: the head's own k = min(300, A) = 21 cuts before max_det = 300 does."""
    cap = 21 * 3
    lists = [make_list(n, cap, 3, 40 + n) for n in (63, 22, 21, 20, 0)]
    det, cnt, _ = run_topk(lists, cap, 21, 300, per_image)
    assert cnt.tolist() == [21, 21, 21, 20, 0]
    check(lists, det, cnt, 21, 300)


def _bits_scores(n, hi_bits, low, seed):
    """Scores that share all but their lowest `low` bits (every radix level above them is degenerate)."""
    g = torch.Generator().manual_seed(seed)
    bits = torch.full((n,), hi_bits, dtype=torch.int32) | torch.randint(0, 1 << low, (n,), generator=g,
                                                                        dtype=torch.int32)
    return bits.view(torch.float32)


@MODES
def test_degenerate_radix_levels_and_ties(per_image):
    cap = 40000
    base = torch.tensor(0.3712).view(torch.int32).item() & ~0xFFF
    lists = [
        make_list(30000, cap, 80, 1, _bits_scores(30000, base, 12, 1)),  # low 12 bits only, many repeats
        make_list(5000, cap, 80, 2, torch.full((5000,), 0.25)),          # all equal: the order is cand_idx
        make_list(300, cap, 80, 3, torch.full((300,), 0.5)),
        make_list(301, cap, 80, 4, torch.full((301,), 0.5)),
    ]
    # duplicated scores across the cut: 295 distinct high scores, then 40 copies of one score over rows 295..334
    hi = torch.linspace(0.99, 0.6, 295)
    lists.append(make_list(335 + 500, cap, 80, 5, torch.cat([hi, torch.full((40,), 0.55), torch.rand(500) * 0.5])))
    det, cnt, _ = run_topk(lists, cap, K, K, per_image)
    check(lists, det, cnt, K, K)
    box, sc, cls, idx = lists[1]
    assert det[1, :, 4].eq(0.25).all() and torch.equal(det[1, :, 5], (idx.sort().values[:K] % 80).float())


@MODES
def test_classes_filter_follows_the_cut(per_image):
    """The filter drops rows after the cut: class 2 has members past the cut that must NOT move up, so the image
    ends with fewer rows of class 2 than candidates of class 2 exist."""
    cap, nc, k = 900, 3, 7
    lists = [make_list(n, cap, nc, 60 + n) for n in (0, 5, 7, 8, 600)]
    for classes in ([2], [0, 2], [1]):
        det, cnt, _ = run_topk(lists, cap, 300, k, per_image, classes=classes)
        check(lists, det, cnt, 300, k, classes=classes)
    det, cnt, _ = run_topk(lists, cap, 300, k, per_image, classes=[2])
    box, sc, cls, idx = lists[-1]
    assert int(cnt[-1]) < k and int((cls == 2).sum()) > k
    for b in range(len(lists)):
        assert det[b, : int(cnt[b]), 5].eq(2).all()


@MODES
def test_record_strides_and_clipping(per_image):
    """One record per image [det | count | pad]: the pad words keep their content, rows past the count are zero;
    boxes are clamped to [0, w] x [0, h]."""
    cap, max_det, pad = 500, 10, 3
    lists = [make_list(n, cap, 3, 80 + n) for n in (0, 4, 10, 400)]
    det, cnt, rec = run_topk(lists, cap, 300, max_det, per_image, clip=(96.0, 160.0), record_pad=pad)
    check(lists, det, cnt, 300, max_det, clip=(96.0, 160.0))
    assert rec[:, max_det * 6 + 1:].eq(-5.0).all()
    live = det[-1, :, :4]
    assert live[:, [0, 2]].max() <= 160.0 and live[:, [1, 3]].max() <= 96.0 and live.min() >= 0.0
    assert (live[:, [0, 2]] == 160.0).any() or (live == 0.0).any()  # the clamp was exercised


def test_entry_point_refuses_bad_descriptors():
    from ydbl import _lib

    fn = _lib.lib.ydbl_detect_topk
    assert fn(None, None) == 1
    p = 0x10000
    ok = dict(cand_box=p, cand_score=p, cand_cls=p, cand_idx=p, cand_count=p, n=1, cap=8, k_head=8, max_det=8, out=p,
              out_count=p, per_image=1)
    for bad, word in ((dict(max_det=0), "max_det"), (dict(max_det=4097), "max_det"), (dict(k_head=0), "k_head"),
                      (dict(out_stride=7), "out_stride"), (dict(per_image=0), "workspace"),
                      (dict(cand_idx=None), "null buffer"), (dict(nclasses=2), "classes")):
        d = _lib.TopkDesc(**{**ok, **bad})
        assert fn(C.byref(d), None) == 1  # refused before any launch: the made-up pointers are never read
        assert word in _lib.lib.ydbl_last_error().decode()


# ----------------------------------------------------------------------------------------------- end2end decode
SHAPES = ((12, 20), (6, 10), (3, 5))  # 96 x 160


def _decode(feats, nc, conf=0.0):
    from ydbl import _lib
    from ydbl.runtime import Plan

    plan = Plan(torch.device(DEV), torch.float32)
    levels = []
    for f in feats:
        n, c, h, w = f.shape
        v = plan.alloc(n, h, w, (c + 7) // 8 * 8).cslice(0, c)  # the box slice's stride in whole 16-byte vectors
        v.torch().copy_(f.permute(0, 2, 3, 1))
        levels.append(v)
    B = feats[0].shape[0]
    A = sum(h * w for h, w in SHAPES)
    cap = A * nc
    yref = torch.full((B, 4 + nc, A), float("nan"), device=DEV)
    cb = torch.empty(B, cap, 4, device=DEV)
    cs = torch.empty(B, cap, device=DEV)
    cc = torch.empty(B, cap, dtype=torch.int32, device=DEV)
    ci = torch.empty(B, cap, dtype=torch.int32, device=DEV)
    cn = torch.empty(B, dtype=torch.int32, device=DEV)
    dd = _lib.DecodeDesc((_lib.View * 3)(*[lv.cslice(0, 64).struct() for lv in levels]),
                         (_lib.View * 3)(*[lv.cslice(64, nc).struct() for lv in levels]), 3, nc,
                         (C.c_float * 3)(8, 16, 32), conf, 1, None, 0, yref.data_ptr(), cb.data_ptr(), cs.data_ptr(),
                         cc.data_ptr(), ci.data_ptr(), cn.data_ptr(), cap)
    plan.launch("ydbl_detect_decode_e2e", dd, keep=[dd])
    plan.run()
    d2 = _lib.DecodeDesc.from_buffer_copy(dd)  # the class-first form: no dense output
    cb2, ci2, cn2 = torch.empty_like(cb), torch.empty_like(ci), torch.empty_like(cn)
    cs2, cc2 = torch.empty_like(cs), torch.empty_like(cc)  # (its own lists: the slot order differs from run to run)
    d2.y_ref, d2.cand_box, d2.cand_idx, d2.cand_count = None, cb2.data_ptr(), ci2.data_ptr(), cn2.data_ptr()
    d2.cand_score, d2.cand_cls = cs2.data_ptr(), cc2.data_ptr()
    p2 = Plan(torch.device(DEV), torch.float32)
    p2.launch("ydbl_detect_decode_e2e", d2, keep=[d2])
    p2.run()
    torch.cuda.synchronize()
    return yref.cpu(), (cb.cpu(), cs.cpu(), cc.cpu(), ci.cpu(), cn.cpu()), (cb2.cpu(), ci2.cpu(), cn2.cpu())


def _head(nc):
    d = U.v10Detect(nc, ch=(16, 16, 16))
    d.stride = torch.tensor([8.0, 16.0, 32.0])
    return d


@pytest.mark.parametrize("nc", [1, 3, 80])
def test_e2e_decode_random_maps(nc):
    """Random level maps: the dense map is [n][4+nc][A] with xyxy rows within the DFL bound of the existing decode
    test (rtol 1e-5, atol 1e-4: expf and the summation order of the 16 bins differ); the candidates at conf 0 are
    every (anchor, class) pair, their boxes the dense map's columns bit for bit, with and without the dense output."""
    g = torch.Generator().manual_seed(nc)
    feats = [torch.randn(2, 64 + nc, h, w, generator=g) * 2 for h, w in SHAPES]
    ref = _head(nc)._inference([f.clone() for f in feats])
    y, (cb, cs, cc, ci, cn), (cb2, ci2, cn2) = _decode(feats, nc)
    A = y.shape[2]
    same = (y[:, :4].view(torch.int32) == ref[:, :4].view(torch.int32)).float().mean().item()
    print(f"nc {nc}: {same:.3f} of the box values bit-equal, max dev {(y - ref).abs().max():.3g}")
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-4)
    assert (y[:, 2] > y[:, 0]).all() and (y[:, 3] > y[:, 1]).all()  # corners, not centre / size
    for b in range(2):
        assert cn[b] == A * nc == cn2[b]
        o = torch.argsort(ci[b])
        assert torch.equal(ci[b][o].long(), torch.arange(A * nc))
        a, j = torch.arange(A * nc) // nc, torch.arange(A * nc) % nc
        assert torch.equal(cc[b][o].long(), j)
        assert torch.equal(cs[b][o], y[b, 4:].T.reshape(-1))
        assert torch.equal(cb[b][o], y[b, :4].T[a])
        assert torch.equal(cb2[b][torch.argsort(ci2[b])], cb[b][o])


@pytest.mark.parametrize("nc", [1, 3])
def test_e2e_decode_bit_equal_where_dfl_is_exact(nc):
    """Box logits whose softmax is exact in fp32 on any implementation -- one bin at 0 and the others at -1e4
    (exp underflows to 0: expectation = the bin), or two bins at 0 (weights 0.5 and 0.5) -- make the DFL expectation
    bit-equal by construction: the boxes must then equal dist2bbox(xywh=False) * stride bit for bit."""
    g = torch.Generator().manual_seed(10 + nc)
    feats = []
    for h, w in SHAPES:
        f = torch.randn(2, 64 + nc, h, w, generator=g)
        box = torch.full((2, 4, 16, h, w), -1e4)
        k1 = torch.randint(0, 16, (2, 4, 1, h, w), generator=g)
        k2 = torch.randint(0, 16, (2, 4, 1, h, w), generator=g)
        box.scatter_(2, k1, 0.0)
        two = torch.rand(2, 4, 1, h, w, generator=g) < 0.5
        box.scatter_(2, torch.where(two, k2, k1), 0.0)
        f[:, :64] = box.reshape(2, 64, h, w)
        feats.append(f)
    head = _head(nc)
    ref = head._inference([f.clone() for f in feats])
    dist = head.dfl(torch.cat([f.view(2, 64 + nc, -1) for f in feats], 2)[:, :64])
    assert torch.equal(dist * 2, (dist * 2).round())  # whole or half bins: exact
    y, (cb, cs, cc, ci, cn), _ = _decode(feats, nc)
    assert torch.equal(y[:, :4], ref[:, :4])
    torch.testing.assert_close(y[:, 4:], ref[:, 4:], rtol=1e-5, atol=1e-6)
