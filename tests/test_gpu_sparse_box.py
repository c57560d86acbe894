"""The sparse box path (include/ydbl.h: the deferred candidate sink of ydbl_dsconv_desc, the tile mask and candidate
sink of ydbl_bottleneck_desc): a Detect level's class tail runs first and flags the 8-row x
16-column tiles that hold an NMS candidate, the level's box launch runs afterwards, on those tiles only, and decodes the
candidates' boxes.

  * the masked box kernel alone: active tiles equal the unmasked launch bit for bit, inactive tiles are not written;
  * deferred tail + masked box against the box launch followed by the tail with the box-reading sink: same counts, same
    lists (sorted by cand_idx) bit for bit, boxes included; the mask is the set of tiles holding a candidate;
  * DetectSession: det / count / cand_count of a sparse_box session equal a keep_pred session's over a sequence of
    batches through one captured graph, and the sessions that must keep their launch plans keep them."""

import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -1234.0  # exact in fp16, far outside the box logits
TH, TW = 8, 16      # the mask granularity


def _cdiv(a, b):
    return -(-a // b)


class _Level:
    """One Detect level: input x [n,h,w,cin], level buffer [n,h,w,64+nc]; the box branch as one pw launch and the class
    branch as one DWConv -> Conv1x1 + class-conv tail launch, both reading x."""

    def __init__(self, n, h, w, cin, nc, seed):
        from ydbl import _lib
        from ydbl.nn import modules as M
        from ydbl.runtime import Plan

        torch.manual_seed(seed)
        self.n, self.h, self.w, self.nc = n, h, w, nc
        self.tx, self.ty = _cdiv(w, TW), _cdiv(h, TH)
        self.plan = Plan(torch.device(DEV), torch.float16)
        self.xv = self.plan.alloc(n, h, w, cin)
        self.xv.torch().copy_(torch.randn(n, h, w, cin).half())
        self.lv = self.plan.alloc(n, h, w, 64 + nc)
        self.lv.torch().zero_()
        c = 64
        ws = [torch.randn(c, cin, 3, 3) / (9 * cin) ** 0.5, torch.randn(c) * 0.5,
              torch.randn(c, c, 3, 3) / (9 * c) ** 0.5, torch.randn(c) * 0.5,
              torch.randn(c, c) / c ** 0.5 * 2, torch.randn(c) * 0.5]
        host = torch.empty(int(_lib.lib.ydbl_detect_box_params_size(cin, c)), dtype=torch.uint8)
        _lib.check(_lib.lib.ydbl_detect_box_pack(*[t.contiguous().data_ptr() for t in ws], cin, c, host.data_ptr()))
        self.params = host.to(DEV)
        self.box = _lib.BottleneckDesc(self.xv.struct(), self.lv.cslice(0, 64).struct(), c, 0, 0,
                                       self.params.data_ptr(), c, 1)
        dwc, pwc, cls = M.DWConv(cin, cin, 3), M.Conv(cin, 64, 1), torch.nn.Conv2d(64, nc, 1)
        with torch.no_grad():
            cls.weight.mul_(8.0)  # scores spread over (0, 1)
        _, done = M.emit_dw_pw(self.plan, dwc, pwc, self.xv, tail_conv=cls, tail_out=self.lv.cslice(64, nc))
        assert done and self.plan.steps[-1].fn.__name__ == "ydbl_dsconv_nhwc"
        self.tail = self.plan.steps[-1].args[0]
        self.mask = torch.ones(n * self.ty * self.tx + 3, dtype=torch.uint8, device=DEV)  # stale 1s, 3 canary bytes

    def run_box(self):
        from ydbl import _lib

        _lib.check(_lib.lib.ydbl_bottleneck_nhwc(self.box, None), "box")

    def run_tail(self):
        from ydbl import _lib

        _lib.check(_lib.lib.ydbl_dsconv_nhwc(self.tail, None), "tail")

    def box_view(self):
        return self.lv.cslice(0, 64).torch()

    def tiles(self, t):
        """[n,h,w,...] -> iterator of (image, tile row, tile column, the tile's slice)."""
        for b in range(self.n):
            for j in range(self.ty):
                for i in range(self.tx):
                    yield b, j, i, t[b, j * TH:(j + 1) * TH, i * TW:(i + 1) * TW]


@pytest.mark.parametrize("h,w", [(20, 24), (9, 17)])
@pytest.mark.parametrize("cin", [64, 128])
def test_masked_box_tiles(cin, h, w):
    """Mask all 0 / all 1 / a seeded mix with both kinds in every image, over a sentinel-filled y: active tiles equal the
    unmasked launch bit for bit, inactive tiles still hold the sentinel.  20x24: tile rows 8 / 8 / 4, columns 16 / 8;
    9x17: a one-row and a one-column tail tile."""
    lvl = _Level(3, h, w, cin, 3, seed=cin + h)
    lvl.run_box()
    torch.cuda.synchronize()
    ref = lvl.box_view().clone()
    assert not bool((ref == SENTINEL).any())
    nt = lvl.ty * lvl.tx
    g = torch.Generator().manual_seed(5)
    mix = (torch.rand(3, nt, generator=g) < 0.5).to(torch.uint8)
    mix[:, 0], mix[:, nt - 1] = torch.tensor([1, 0, 1], dtype=torch.uint8), torch.tensor([0, 1, 0], dtype=torch.uint8)
    for m in (torch.zeros(3, nt, dtype=torch.uint8), torch.ones(3, nt, dtype=torch.uint8), mix):
        mask = m.reshape(-1).to(DEV)
        lvl.box_view().fill_(SENTINEL)
        lvl.box.tile_mask = mask.data_ptr()
        lvl.run_box()
        torch.cuda.synchronize()
        got = lvl.box_view()
        m3 = m.view(3, lvl.ty, lvl.tx)
        for (b, j, i, tg), (_, _, _, tr) in zip(lvl.tiles(got), lvl.tiles(ref)):
            if m3[b, j, i]:
                assert torch.equal(tg, tr), (b, j, i)
            else:
                assert bool((tg == SENTINEL).all()), (b, j, i)
    lvl.box.tile_mask = None
    assert not bool(lvl.lv.cslice(64, 3).torch().any())  # the class slice is untouched


def test_sparse_box_descriptor_rules():
    from ydbl import _lib

    lvl = _Level(1, 9, 17, 64, 3, seed=1)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    lvl.box.cand_count = cnt.data_ptr()  # a sink without a mask
    assert _lib.lib.ydbl_bottleneck_nhwc(lvl.box, None) == 1
    lvl.box.cand_count, lvl.box.tile_mask, lvl.box.pw = None, lvl.mask.data_ptr(), 0  # a mask without pw
    assert _lib.lib.ydbl_bottleneck_nhwc(lvl.box, None) == 1
    lvl.tail.tile_mask = lvl.mask.data_ptr()  # a mask without a sink
    assert _lib.lib.ydbl_dsconv_nhwc(lvl.tail, None) == 1


A0, STRIDE = 7, 8.0  # the level's first anchor (not 0: the box launch filters by the level's anchor range) and stride


def _buffers(n, cap, canary=4):
    """The five candidate arrays with `canary` extra rows of a fill value behind the n * cap entries."""
    rows = n * cap + canary
    return [torch.full((rows, 4), 7.5, device=DEV), torch.full((rows,), 7.5, device=DEV),
            torch.full((rows,), -77, dtype=torch.int32, device=DEV), torch.full((rows,), -77, dtype=torch.int32, device=DEV),
            torch.full((n,), 12345, dtype=torch.int32, device=DEV)]  # stale counts: the call must zero them


def _set_sink(lvl, bufs, cap, conf, multi, classes, deferred):
    d, b = lvl.tail, lvl.box
    d.cand_box, d.cand_score, d.cand_cls, d.cand_idx, d.cand_count = [t.data_ptr() for t in bufs]
    d.cand_cap, d.conf_thres, d.multi_label = cap, conf, multi
    d.classes, d.nclasses = (classes.data_ptr(), len(classes)) if classes is not None else (None, 0)
    d.level_stride, d.anchor0, d.box, d.zero_counts = STRIDE, A0, lvl.lv.cslice(0, 64).struct(), 1
    if deferred:
        d.tile_mask, d.mask_tiles_x, d.mask_tiles_img = lvl.mask.data_ptr(), lvl.tx, lvl.tx * lvl.ty
        d.mask_zero, d.mask_zero_bytes = lvl.mask.data_ptr(), lvl.n * lvl.tx * lvl.ty
        b.tile_mask = lvl.mask.data_ptr()
        b.cand_box, b.cand_idx, b.cand_count, b.cand_cap = bufs[0].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), cap
        b.level_stride, b.anchor0, b.nc, b.multi_label = STRIDE, A0, lvl.nc, multi
    else:
        d.tile_mask, d.mask_zero, d.mask_zero_bytes = None, None, 0
        b.tile_mask, b.cand_count = None, None


def _pair(lvl, cap, conf, multi, classes, deferred):
    """Today's pair (box launch, then the tail with the box-reading sink) or the sparse pair (deferred tail, then the
    masked box launch with the candidate sink) over a sentinel-filled box slice; the candidate arrays on the host."""
    bufs = _buffers(lvl.n, cap)
    lvl.box_view().fill_(SENTINEL)
    lvl.mask.fill_(1)
    _set_sink(lvl, bufs, cap, conf, multi, classes, deferred)
    if deferred:
        lvl.run_tail()
        lvl.run_box()
    else:
        lvl.run_box()
        lvl.run_tail()
    torch.cuda.synchronize()
    return [t.cpu() for t in bufs]


def _host_mask(lvl, idx, cnt, cap, multi):
    """The tiles that hold a candidate, from a candidate list."""
    m = torch.zeros(lvl.n, lvl.ty, lvl.tx, dtype=torch.uint8)
    for b in range(lvl.n):
        for a in idx[b * cap:b * cap + min(int(cnt[b]), cap)].tolist():
            loc = (a // lvl.nc if multi else a) - A0
            assert 0 <= loc < lvl.h * lvl.w
            m[b, (loc // lvl.w) // TH, (loc % lvl.w) // TW] = 1
    return m


def _assert_same_lists(got, ref, n, cap):
    gb, gs, gc, gi, gn = got
    rb, rs, rc, ri, rn = ref
    assert torch.equal(gn, rn), (gn.tolist(), rn.tolist())
    for b in range(n):
        k = min(int(rn[b]), cap)
        sl = slice(b * cap, b * cap + k)
        og, orf = torch.argsort(gi[sl]), torch.argsort(ri[sl])
        assert torch.equal(gi[sl][og], ri[sl][orf])
        assert torch.equal(gc[sl][og], rc[sl][orf])
        assert torch.equal(gs[sl][og].view(torch.int32), rs[sl][orf].view(torch.int32))
        assert torch.equal(gb[sl][og].view(torch.int32), rb[sl][orf].view(torch.int32))


def _scores(lvl):
    """sigmoid of the stored class logits [n, h*w, nc] (threshold picking)."""
    lvl.tail.cand_count = None
    lvl.run_tail()
    torch.cuda.synchronize()
    return lvl.lv.cslice(64, lvl.nc).torch().float().reshape(lvl.n, -1, lvl.nc).sigmoid().cpu()


@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("cin", [64, 128])
def test_deferred_tail_and_masked_box_equal_todays_pair(cin, nc):
    """Map 20x24 (18 tiles over 3 images), the threshold at the 9th largest anchor score, so that a few tiles hold a
    candidate and most do not (asserted); single-label, multi-label, and both with a class filter.  cin 64: the
    one-round-trip tail tile, 128: the chunked kernel."""
    n, h, w = 3, 20, 24
    lvl = _Level(n, h, w, cin, nc, seed=10 * cin + nc)
    best = _scores(lvl).max(2).values
    conf = float(best.flatten().sort().values[-9])
    flt = torch.tensor([nc - 1, 0] if nc > 2 else [0], dtype=torch.int32, device=DEV)
    for multi, classes in ((0, None), (1, None), (0, flt), (1, flt)):
        multi = int(bool(multi) and nc > 1)
        cap = (A0 + h * w + 5) * (nc if multi else 1)
        ref = _pair(lvl, cap, conf, multi, classes, deferred=False)
        box_ref = lvl.box_view().clone()
        got = _pair(lvl, cap, conf, multi, classes, deferred=True)
        _assert_same_lists(got, ref, n, cap)
        for t, r in zip(got[:4], ref[:4]):  # nothing behind the lists
            assert torch.equal(t[n * cap:], r[n * cap:])
        want = _host_mask(lvl, ref[3], ref[4], cap, multi)
        mask = lvl.mask.cpu()
        assert torch.equal(mask[:n * lvl.ty * lvl.tx].view(n, lvl.ty, lvl.tx), want)
        assert mask[n * lvl.ty * lvl.tx:].tolist() == [1, 1, 1]  # the bytes behind the mask keep their fill
        assert 0 < int(want.sum()) < want.numel(), "the threshold must leave both kinds of tile"
        for (b, j, i, tg), (_, _, _, tr) in zip(lvl.tiles(lvl.box_view()), lvl.tiles(box_ref)):
            assert torch.equal(tg, tr) if want[b, j, i] else bool((tg == SENTINEL).all()), (b, j, i)


def test_deferred_pair_overflow():
    """cap below the count (conf 0: every anchor a candidate): the counts are the full ones, nothing is written behind
    the lists, and every kept entry is a candidate of the reference with that candidate's score, class and box."""
    n, h, w, nc = 3, 20, 24, 3
    lvl = _Level(n, h, w, 64, nc, seed=99)
    full = A0 + h * w
    ref = _pair(lvl, full, 0.0, 0, None, deferred=False)
    assert ref[4].tolist() == [h * w] * n
    cap = 100
    got = _pair(lvl, cap, 0.0, 0, None, deferred=True)
    assert got[4].tolist() == [h * w] * n
    assert bool((got[0][n * cap:] == 7.5).all()) and bool((got[1][n * cap:] == 7.5).all())
    assert bool((got[2][n * cap:] == -77).all()) and bool((got[3][n * cap:] == -77).all())
    for b in range(n):
        by_idx = {int(i): k for k, i in enumerate(ref[3][b * full:b * full + h * w].tolist())}
        kept = got[3][b * cap:(b + 1) * cap].tolist()
        assert len(set(kept)) == cap
        for s, a in enumerate(kept):
            k = b * full + by_idx[a]
            assert int(got[2][b * cap + s]) == int(ref[2][k])
            assert torch.equal(got[1][b * cap + s].view(torch.int32), ref[1][k].view(torch.int32))
            assert torch.equal(got[0][b * cap + s].view(torch.int32), ref[0][k].view(torch.int32))


# ------------------------------------------------------------------------------------------------ sessions
def _yolo(golden_dir, cfg="yolov13n_DBL.yaml", fx="trained_yolov13n_DBL_nc3.npz"):
    from ydbl import YOLO
    from ydbl.utils.synthetic import load_trained

    torch.manual_seed(0)
    m = YOLO(cfg, nc=3)
    load_trained(m.model, golden_dir / fx)
    return m


def _whats(s):
    return [[st.what for st in c.plan.steps] for c in (s.children or [s])]


@pytest.fixture
def no_sparse_env():
    def set_(on):
        if on:
            os.environ["YDBL_NO_SPARSE_BOX"] = "1"
        else:
            os.environ.pop("YDBL_NO_SPARSE_BOX", None)
    yield set_
    os.environ.pop("YDBL_NO_SPARSE_BOX", None)


@pytest.mark.parametrize("streams", [1, 2])
def test_session_equals_keep_pred_session(streams, golden_dir):
    """DBL-n, batch 3 at 256^2, conf 0.25: batches seed 6 (every image has candidates, some P3 tiles without), seed 5
    (images 1 and 2 have none), seed 6 again through the same captured graph -- a mask byte or a counter left over
    from the batch before would show as a difference from the keep_pred session (decode pass, full box maps)."""
    from ydbl.utils.synthetic import blob_images

    m = _yolo(golden_dir)
    s = m.session(3, 256, 256, half=True, conf=0.25, iou=0.7, streams=streams)
    r = m.session(3, 256, 256, half=True, conf=0.25, iou=0.7, streams=streams, keep_pred=True)
    assert s.sparse_box and not r.sparse_box
    for c in (s.children or [s]):
        what = [st.what for st in c.plan.steps]
        boxes = [k for k, w_ in enumerate(what) if w_ == "Detect.box3"]
        assert len(boxes) == 2  # P3, P4
        for k in boxes:  # the box launch right behind the level's class tail
            assert c.plan.steps[k - 1].fn.__name__ == "ydbl_dsconv_nhwc" and c.plan.steps[k - 1].args[0].tail_w
            assert c.plan.steps[k - 1].args[0].tile_mask == c.plan.steps[k].args[0].tile_mask
    for seed in (6, 5, 6):
        x = blob_images(3, 256, seed=seed).to(DEV)
        s(x)
        r(x)
        torch.cuda.synchronize()
        cnt = r.cand_count.cpu()
        print(f"seed {seed}: candidates {cnt.tolist()} detections {r.count.cpu().tolist()}")
        assert torch.equal(s.cand_count.cpu(), cnt)
        assert torch.equal(s.count.cpu(), r.count.cpu())
        assert torch.equal(s.det.cpu().view(torch.int32), r.det.cpu().view(torch.int32))
        if seed == 6:
            assert int(cnt.min()) > 0
        else:
            assert cnt.tolist()[1:] == [0, 0]
        for c in (s.children or [s]):  # the masks: exactly the tiles of this batch's candidates
            lo = [0, 32 * 32]  # P3 / P4 first anchors at 256^2
            k = min(int(c.cand_count.max()), c.cand_idx.shape[1])
            idx, n_ = c.cand_idx[:, :k].cpu(), c.cand_count.cpu().tolist()
            for lv, mk in c.tile_masks.items():
                hw = (256 // (8 << lv))
                want = torch.zeros_like(mk, device="cpu")
                for b in range(idx.shape[0]):
                    for a in idx[b, :n_[b]].tolist():
                        loc = a - lo[lv]
                        if 0 <= loc < hw * hw:
                            want[b, (loc // hw) // TH, (loc % hw) // TW] = 1
                assert torch.equal(mk.cpu(), want), (seed, lv)
        if seed == 6:  # the active tiles per image the CPU oracle gives for this batch: P3 3 / 1 / 2 of 8, P4 2 of 2
            per = {lv: [int(v) for c in (s.children or [s]) for v in c.tile_masks[lv].flatten(1).sum(1).tolist()]
                   for lv in (0, 1)}
            assert per == {0: [3, 1, 2], 1: [2, 2, 2]}, per


def test_other_sessions_keep_their_plans(golden_dir, no_sparse_env):
    """YDBL_NO_SPARSE_BOX=1, conf below the per-image-NMS threshold and fp8 keep the launch order of a session without
    the path; DBL-s (no one-launch box branch) is the same plan with and without the switch."""
    m = _yolo(golden_dir)
    sparse = m.session(3, 256, 256, half=True, conf=0.25, iou=0.7, streams=1)
    assert sparse.sparse_box
    no_sparse_env(True)
    base = m.session(3, 256, 256, half=True, conf=0.25, iou=0.7, streams=1)
    no_sparse_env(False)
    assert not base.sparse_box and base.fused_candidates
    w0 = _whats(base)
    assert _whats(sparse) != w0 and sorted(_whats(sparse)[0]) == sorted(w0[0])
    for st in base.plan.steps:
        d = st.args[0] if st.args else None
        assert not getattr(d, "tile_mask", None) and not getattr(d, "mask_zero", None)
    low = m.session(3, 256, 256, half=True, conf=0.05, iou=0.7, streams=1)
    assert not low.sparse_box and _whats(low) == w0
    q = m.session(3, 256, 256, half=True, conf=0.25, iou=0.7, streams=1, fp8=True)
    assert not q.sparse_box and _whats(q) == w0
    with pytest.warns(UserWarning, match="not computed"):
        sparse.feats()
    ms = _yolo(golden_dir, "yolov13s_DBL.yaml", "trained_yolov13s_DBL_nc3.npz")
    a = ms.session(3, 256, 256, half=True, conf=0.25, iou=0.7, streams=1)
    no_sparse_env(True)
    b = ms.session(3, 256, 256, half=True, conf=0.25, iou=0.7, streams=1)
    assert not a.sparse_box and not b.sparse_box and _whats(a) == _whats(b)


def test_bench_batch_equals_plan_without_the_path(golden_dir, no_sparse_env):
    """The benchmark's workload (DBL-n 640^2 bs32 fp16, two sub-batch graphs, blob_images seed 1234): det and count equal
    the session built under YDBL_NO_SPARSE_BOX=1 bit for bit, and the candidate statistics are the benchmark's."""
    from ydbl.utils.synthetic import blob_images

    m = _yolo(golden_dir)
    x = blob_images(32, 640, seed=1234).to(DEV)
    s = m.session(32, 640, 640, half=True, conf=0.25, iou=0.7, max_det=300, streams=2)
    assert s.sparse_box
    s(x)
    torch.cuda.synchronize()
    det, count, cand = s.det.cpu().clone(), s.count.cpu().clone(), s.cand_count.cpu().clone()
    active = [torch.cat([c.tile_masks[lv].flatten() for c in s.children]).float().mean().item() for lv in (0, 1)]
    print(f"share of box workgroups that run: P3 {active[0]:.3f} P4 {active[1]:.3f}")
    del s
    m.reset_sessions()
    no_sparse_env(True)
    r = m.session(32, 640, 640, half=True, conf=0.25, iou=0.7, max_det=300, streams=2)
    assert not r.sparse_box
    r(x)
    torch.cuda.synchronize()
    assert torch.equal(cand, r.cand_count.cpu()) and torch.equal(count, r.count.cpu())
    assert torch.equal(det.view(torch.int32), r.det.cpu().view(torch.int32))
    assert round(float(cand.float().mean()), 1) == 121.3 and int(cand.max()) == 645
