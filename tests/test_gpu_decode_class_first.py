"""ydbl_detect_decode without y_ref evaluates the classes first and decodes a box only where a quad holds a candidate
(csrc/decode_math.hpp, quad_candidates); with y_ref it decodes every anchor's box first, as it always did.  Both
must offer the same candidates: equal counts and equal (idx, cls, score bits, box bits) sets.  The y_ref pass is
pinned bit for bit to what it offers: a candidate's score is y_ref's score of its (class, anchor), and its box is
xywh2xyxy (U/utils/ops.py:416-433) of y_ref's xywh column in IEEE fp32."""

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAPS = ((20, 20), (5, 7), (8, 8))
A = sum(h * w for h, w in MAPS)


def _decode(levels, n, nc, conf, multi, classes, with_yref):
    from ydbl import _lib

    cap = A * nc if multi else A
    bufs = [torch.zeros(n, cap, 4, device=DEV), torch.zeros(n, cap, device=DEV),
            torch.zeros(n, cap, dtype=torch.int32, device=DEV), torch.zeros(n, cap, dtype=torch.int32, device=DEV),
            torch.full((n,), 777, dtype=torch.int32, device=DEV)]
    yref = torch.zeros(n, 4 + nc, A, device=DEV) if with_yref else None
    dd = _lib.DecodeDesc((_lib.View * 3)(*[lv.cslice(0, 64).struct() for lv in levels]),
                         (_lib.View * 3)(*[lv.cslice(64, nc).struct() for lv in levels]), 3, nc,
                         (C.c_float * 3)(8, 16, 32), conf, multi, classes.data_ptr() if classes is not None else None,
                         len(classes) if classes is not None else 0, yref.data_ptr() if with_yref else None,
                         *[t.data_ptr() for t in bufs], cap)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib.ydbl_detect_decode(dd, s), "decode")
    torch.cuda.synchronize()
    return bufs, yref, cap


@pytest.mark.parametrize("nc", [1, 3, 4, 7])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_class_first_equals_box_first(dtype, n, nc):
    from ydbl.runtime import Plan

    g = torch.Generator().manual_seed(1000 * n + 10 * nc + (dtype == torch.float16))
    plan = Plan(torch.device(DEV), dtype)
    levels = []
    for h, w in MAPS:
        lv = plan.alloc(n, h, w, 64 + nc)
        lv.torch().copy_((torch.randn(n, h, w, 64 + nc, generator=g) * 2).to(dtype))
        levels.append(lv)
    flt = torch.tensor([nc - 1, 0] if nc > 2 else [0], dtype=torch.int32, device=DEV)
    # single-label: no anchor (a sigmoid is <= 1), some, every anchor (cap = A exactly full); multi-label +- filter
    for conf, multi, classes, expect in ((1.0, 0, None, "none"), (0.6, 0, None, "some"), (0.0, 0, None, "all"),
                                         (0.6, 0, flt, None), (0.6, 1, None, "some"), (0.6, 1, flt, "some")):
        (rb, rs, rc, ri, rn), yref, cap = _decode(levels, n, nc, conf, multi, classes, True)
        (gb, gs, gc, gi, gn), _, _ = _decode(levels, n, nc, conf, multi, classes, False)
        assert torch.equal(gn, rn), (gn.tolist(), rn.tolist())
        cnt = rn.cpu()
        if expect == "none":
            assert int(cnt.sum()) == 0
        elif expect == "all":
            assert cnt.tolist() == [A] * n
        elif expect == "some":
            assert 0 < int(cnt.min()) and int(cnt.max()) < cap
        for b in range(n):
            k = int(rn[b])
            og, orf = torch.argsort(gi[b, :k]), torch.argsort(ri[b, :k])
            idx, cls = ri[b, :k][orf].long(), rc[b, :k][orf].long()
            assert torch.equal(gi[b, :k][og].long(), idx) and torch.equal(gc[b, :k][og].long(), cls)
            assert torch.equal(gs[b, :k][og].view(torch.int32), rs[b, :k][orf].view(torch.int32))
            assert torch.equal(gb[b, :k][og].view(torch.int32), rb[b, :k][orf].view(torch.int32))
            # the y_ref pass against its own prediction tensor, bit for bit
            anchor = idx // nc if multi else idx
            y = yref[b].cpu()
            a_c, c_c = anchor.cpu(), cls.cpu()
            assert torch.equal(y[4 + c_c, a_c].view(torch.int32), rs[b, :k][orf].cpu().view(torch.int32))
            cx, cy, hw, hh = y[0, a_c], y[1, a_c], y[2, a_c] / 2.0, y[3, a_c] / 2.0
            box = torch.stack([cx - hw, cy - hh, cx + hw, cy + hh], 1)
            assert torch.equal(box.view(torch.int32), rb[b, :k][orf].cpu().view(torch.int32))
            if not multi:  # single-label: the first maximum over the classes
                best, bj = y[4:].max(0)
                assert torch.equal(bj[a_c], c_c)
