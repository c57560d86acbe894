"""The class-conv tail of ydbl_dsconv_nhwc as the source of the NMS candidates (include/ydbl.h, the candidate sink of
ydbl_dsconv_desc), through the C ABI: three Detect levels launched with the sink set against the same three
launches without it followed by ydbl_detect_decode on the same buffers.  Counts per image equal, and the
(idx, cls, score bits, box bits) tuples equal after sorting by idx -- candidate order within an image is free.

Maps 20x20 (ragged against the 8x8 tile), 5x7 and 8x8; the class pair's input channels 64 (the one-round-trip
tile) and 128 (the chunked kernel), level 2 at 256 (chunked: the 256-channel lean tile holds no tail)."""

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAPS = ((20, 20), (5, 7), (8, 8))
STRIDES = (8.0, 16.0, 32.0)
A = sum(h * w for h, w in MAPS)


class _Head:
    """Three level buffers [n,h,w,64+nc] with random box logits, and per level one DWConv -> Conv1x1 (+ class conv
    tail) launch writing the class slice; cands(...) runs them with or without the sink."""

    def __init__(self, chans, n, nc, seed):
        from ydbl.nn import modules as M
        from ydbl.runtime import Plan

        torch.manual_seed(seed)
        self.n, self.nc = n, nc
        self.plan = Plan(torch.device(DEV), torch.float16)
        self.levels, self.descs, self.ys = [], [], []
        for (h, w), cin in zip(MAPS, chans):
            dwc, pwc, cls = M.DWConv(cin, cin, 3), M.Conv(cin, 64, 1), torch.nn.Conv2d(64, nc, 1)
            with torch.no_grad():
                cls.weight.mul_(8.0)  # scores spread over (0, 1)
            xv = self.plan.alloc(n, h, w, cin)
            xv.torch().copy_(torch.randn(n, h, w, cin).half())
            lv = self.plan.alloc(n, h, w, 64 + nc)
            lv.torch().zero_()
            lv.cslice(0, 64).torch().copy_((torch.randn(n, h, w, 64) * 2).half())
            y, done = M.emit_dw_pw(self.plan, dwc, pwc, xv, tail_conv=cls, tail_out=lv.cslice(64, nc))
            assert done and self.plan.steps[-1].fn.__name__ == "ydbl_dsconv_nhwc"
            self.levels.append(lv)
            self.ys.append(y)
            self.descs.append(self.plan.steps[-1].args[0])
        self.tail_steps = list(self.plan.steps)

    def buffers(self, cap):
        n = self.n
        return [torch.zeros(n, cap, 4, device=DEV), torch.zeros(n, cap, device=DEV),
                torch.zeros(n, cap, dtype=torch.int32, device=DEV), torch.zeros(n, cap, dtype=torch.int32, device=DEV),
                torch.full((n,), 12345, dtype=torch.int32, device=DEV)]  # stale counts: the call must zero them

    def decode_desc(self, bufs, cap, conf, multi, classes):
        from ydbl import _lib

        return _lib.DecodeDesc((_lib.View * 3)(*[lv.cslice(0, 64).struct() for lv in self.levels]),
                               (_lib.View * 3)(*[lv.cslice(64, self.nc).struct() for lv in self.levels]), 3, self.nc,
                               (C.c_float * 3)(*STRIDES), conf, multi,
                               classes.data_ptr() if classes is not None else None,
                               len(classes) if classes is not None else 0, None, *[t.data_ptr() for t in bufs], cap)

    def set_sink(self, dd):
        a0 = 0
        for i, (d, (h, w)) in enumerate(zip(self.descs, MAPS)):
            if dd is None:
                d.cand_count = None
                continue
            d.cand_box, d.cand_score, d.cand_cls = dd.cand_box, dd.cand_score, dd.cand_cls
            d.cand_idx, d.cand_count, d.cand_cap = dd.cand_idx, dd.cand_count, dd.cap
            d.conf_thres, d.multi_label, d.classes, d.nclasses = dd.conf_thres, dd.multi_label, dd.classes, dd.nclasses
            d.level_stride, d.anchor0, d.box, d.zero_counts = STRIDES[i], a0, dd.box[i], int(i == 0)
            a0 += h * w

    def run(self, extra=()):
        from ydbl.runtime import Step

        self.plan.steps = self.tail_steps + [Step(*e) for e in extra]
        self.plan.run()
        torch.cuda.synchronize()

    def cands(self, fused, conf, multi, classes=None, cap=None):
        from ydbl import _lib

        cap = cap or (A * self.nc if multi else A)
        bufs = self.buffers(cap)
        dd = self.decode_desc(bufs, cap, conf, multi, classes)
        if fused:
            self.set_sink(dd)
            self.run()
            self.set_sink(None)
        else:
            self.run([(_lib.lib.ydbl_detect_decode, (dd,), "decode", [dd])])
        return bufs

    def scores(self):
        """Per level-concatenated anchor: sigmoid of the stored class logits, [n, A, nc] fp32 (threshold picking)."""
        self.run()
        return torch.cat([lv.cslice(64, self.nc).torch().float().reshape(self.n, -1, self.nc) for lv in self.levels],
                         1).sigmoid().cpu()


def _assert_same(got, ref, n, cap):
    gb, gs, gc, gi, gn = got
    rb, rs, rc, ri, rn = ref
    assert torch.equal(gn, rn), (gn.tolist(), rn.tolist())
    for b in range(n):
        k = min(int(rn[b]), cap)
        og, orf = torch.argsort(gi[b, :k]), torch.argsort(ri[b, :k])
        assert torch.equal(gi[b, :k][og], ri[b, :k][orf])
        assert torch.equal(gc[b, :k][og], rc[b, :k][orf])
        assert torch.equal(gs[b, :k][og].view(torch.int32), rs[b, :k][orf].view(torch.int32))
        assert torch.equal(gb[b, :k][og].view(torch.int32), rb[b, :k][orf].view(torch.int32))


@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("c", [64, 128])
def test_tail_candidates_equal_decode(c, n, nc):
    """Single-label at thresholds no anchor / some anchors / every anchor passes (conf 0 with cap = A: the capacity
    edge), multi-label with and without a classes filter."""
    hd = _Head((c, c, 256), n, nc, seed=100 * c + 10 * n + nc)
    best = hd.scores().max(2).values
    assert float(best.min()) > 0.0
    some = float(best.flatten().sort().values[best.numel() // 2])
    flt = torch.tensor([nc - 1, 0] if nc > 2 else [0], dtype=torch.int32, device=DEV)
    for conf, multi, classes, expect in ((1.0, 0, None, "none"), (some, 0, None, "some"),  # (a sigmoid is <= 1)
                                         (0.0, 0, None, "all"), (some, 1, None, "some"), (some, 1, flt, "some"),
                                         (some, 0, flt, None)):
        cap = A * nc if multi else A
        ref = hd.cands(False, conf, multi, classes)
        got = hd.cands(True, conf, multi, classes)
        _assert_same(got, ref, n, cap)
        cnt = ref[4].cpu()
        if expect == "none":
            assert int(cnt.sum()) == 0
        elif expect == "all":
            assert cnt.tolist() == [A] * n
        elif expect == "some":
            assert 0 < int(cnt.min()) and int(cnt.max()) < cap


def test_tail_candidates_replayed_in_a_graph():
    """The same descriptors launched twice inside one captured graph, replayed twice: the counts are one call's --
    the first level's launch zeroes the counters every time, no state is carried between calls."""
    hd = _Head((64, 128, 256), 2, 3, seed=7)
    best = hd.scores().max(2).values
    conf = float(best.flatten().sort().values[best.numel() // 2])
    ref = hd.cands(False, conf, 0)
    bufs = hd.buffers(A)
    dd = hd.decode_desc(bufs, A, conf, 0, None)
    hd.set_sink(dd)
    hd.run()  # eager once: modules loaded before the capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        hd.plan.run()
        hd.plan.run()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        _assert_same(bufs, ref, 2, A)
    assert 0 < int(ref[4].min())


def test_tail_y_unused_leaves_y_alone():
    """y_unused on the 64 -> 64 tail launch: class logits and candidates as with y written, and a sentinel-filled y
    buffer is unchanged afterwards."""
    hd = _Head((64, 64, 64), 3, 3, seed=11)
    best = hd.scores().max(2).values
    conf = float(best.flatten().sort().values[best.numel() // 2])
    ref = hd.cands(True, conf, 0)
    cls_ref = [lv.cslice(64, 3).torch().clone() for lv in hd.levels]
    y_ref = [y.torch().clone() for y in hd.ys]
    for lv in hd.levels:
        lv.cslice(64, 3).torch().zero_()
    for y, d in zip(hd.ys, hd.descs):
        y.torch().fill_(7.0)
        d.y_unused = 1
    got = hd.cands(True, conf, 0)
    _assert_same(got, ref, 3, A)
    assert 0 < int(ref[4].min())
    for lv, r in zip(hd.levels, cls_ref):
        assert torch.equal(lv.cslice(64, 3).torch(), r)
    for y, r in zip(hd.ys, y_ref):
        assert bool((y.torch() == 7.0).all()) and not bool((r == 7.0).all())
