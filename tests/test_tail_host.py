"""ydbl.tail without a GPU: the candidate lists on the meta device, and decode_desc against a descriptor written out by
hand on host tensors (real addresses, nothing launched)."""

import ctypes as C

import pytest
import torch


@pytest.mark.parametrize("A, nc, multi, cap", [(252, 3, False, 252), (252, 3, True, 756), (252, 1, True, 252)])
def test_candidate_lists(A, nc, multi, cap):
    from ydbl.runtime import Plan
    from ydbl.tail import CandidateLists

    assert CandidateLists.capacity(A, nc, multi) == cap
    plan = Plan("meta", torch.float16)
    c = CandidateLists(2, cap, "meta", plan)
    lists = [c.box, c.score, c.cls, c.idx, c.count]
    assert [tuple(t.shape) for t in lists] == [(2, cap, 4), (2, cap), (2, cap), (2, cap), (2,)]
    assert [t.dtype for t in lists] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.int32]
    assert all(t.device.type == "meta" for t in lists)
    assert len(plan.buffers) == 5 and all(a is b for a, b in zip(plan.buffers, lists))
    assert list(c.fields()) == ["cand_box", "cand_score", "cand_cls", "cand_idx", "cand_count", "cap"]
    assert c.fields()["cap"] == cap
    assert CandidateLists(2, cap, "cpu").count.tolist() == [0, 0]  # (no plan: nothing to register; zero-filled)


def _same(a, b, tp):
    if issubclass(tp, C.Array):
        return all(_same(x, y, tp._type_) for x, y in zip(a, b))
    if issubclass(tp, C.Structure):
        return all(_same(getattr(a, n), getattr(b, n), t) for n, t in tp._fields_)
    return a == b


@pytest.mark.parametrize("nc, multi, with_classes, with_pred", [(3, True, True, True), (1, False, False, False)])
def test_decode_desc_equals_the_hand_written_descriptor(nc, multi, with_classes, with_pred):
    from ydbl import _lib
    from ydbl.runtime import Plan
    from ydbl.tail import CandidateLists, decode_desc

    plan = Plan("cpu", torch.float16)
    levels = [plan.alloc(2, h, w, 64 + nc) for h, w in ((12, 16), (6, 8), (3, 4))]
    A = sum(lv.h * lv.w for lv in levels)
    cands = CandidateLists(2, CandidateLists.capacity(A, nc, multi), "cpu", plan)
    ct = torch.tensor([0, 2], dtype=torch.int32) if with_classes else None
    pred = torch.empty((2, 4 + nc, A), dtype=torch.float32) if with_pred else None
    got = decode_desc(levels, [8.0, 16.0, 32.0], nc, 16, 0.25, multi, ct, pred, cands)
    want = _lib.DecodeDesc((_lib.View * 3)(*[lv.cslice(0, 64).struct() for lv in levels]),
                           (_lib.View * 3)(*[lv.cslice(64, nc).struct() for lv in levels]), 3, nc,
                           (C.c_float * 3)(8.0, 16.0, 32.0), 0.25, int(multi),
                           ct.data_ptr() if ct is not None else None, len(ct) if ct is not None else 0,
                           pred.data_ptr() if pred is not None else None, cands.box.data_ptr(),
                           cands.score.data_ptr(), cands.cls.data_ptr(), cands.idx.data_ptr(), cands.count.data_ptr(),
                           cands.cap)
    for name, tp in _lib.DecodeDesc._fields_:
        assert _same(getattr(got, name), getattr(want, name), tp), name
    assert got.cand_box and got.cand_count and got.cls[2].ptr == levels[2].ptr + 64 * 2  # (real addresses)
    assert got.cap == (A * nc if multi and nc > 1 else A)
