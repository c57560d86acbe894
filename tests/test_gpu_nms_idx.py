"""ydbl_nms's optional out_idx on the MI355X: row k of an image receives the kept candidate's cand_idx, rows past the
count -1, and out / out_count are what they are without it.

n = 2 images with 64 and 600 candidates of 3 classes (600 is above one 512-thread pass, 64 below), in list order
shuffled, boxes clustered so that the NMS drops a good share.  Both schedules (per_image 0: the class-split sweep
plus nms_merge_kernel; 1: the sweep's own write) and agnostic 0 / 1 (agnostic always takes the sweep's write), with
single-label (cand_idx = anchor) and multi-label (cand_idx = anchor * nc + cls, several classes of one anchor) lists."""

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NC, CAP, MAX_DET = 3, 1500, 300
CLIP = (120.0, 160.0)  # (h, w): some boxes reach outside


def make_list(n, seed, multi):
    """(box [n,4], score [n], cls [n], idx [n]) in shuffled list order; idx distinct."""
    g = torch.Generator().manual_seed(seed)
    if multi:  # anchors with 1..3 classes each, one box per anchor
        anchors = torch.randperm(CAP // NC, generator=g)
        rows = []
        for a in anchors.tolist():
            k = int(torch.randint(1, NC + 1, (1,), generator=g))
            for c in torch.randperm(NC, generator=g)[:k].tolist():
                rows.append((a, c))
            if len(rows) >= n:
                break
        rows = rows[:n]
        anc = torch.tensor([r[0] for r in rows])
        cls = torch.tensor([r[1] for r in rows], dtype=torch.int32)
        idx = (anc * NC + cls).int()
    else:
        anc = torch.randperm(CAP, generator=g)[:n]
        cls = torch.randint(0, NC, (n,), generator=g).int()
        idx = anc.int()
    # per anchor: a box near one of n / 4 cluster centres, of about the cluster's size: boxes of one class overlap
    k = max(n // 4, 1)
    cc, cwh = torch.rand(k, 2, generator=g) * torch.tensor([170.0, 130.0]) - 5.0, torch.rand(k, 2, generator=g) * 40 + 8
    of = torch.randint(0, k, (CAP,), generator=g)
    ctr = cc[of] + torch.randn(CAP, 2, generator=g) * 2.0
    wh = cwh[of] * (1 + 0.1 * torch.randn(CAP, 2, generator=g)).clamp(0.7, 1.3)
    box = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)[anc]
    score = (torch.rand(n, generator=g) * 0.9 + 0.05).float()
    perm = torch.randperm(n, generator=g)
    return box[perm], score[perm], cls[perm], idx[perm]


def run_nms(lists, per_image, agnostic, with_idx):
    from ydbl import _lib

    B = len(lists)
    cb = torch.full((B, CAP, 4), float("nan"))
    cs = torch.full((B, CAP), float("nan"))
    cc = torch.full((B, CAP), -7, dtype=torch.int32)
    ci = torch.full((B, CAP), -3, dtype=torch.int32)
    cn = torch.zeros(B, dtype=torch.int32)
    for b, (box, sc, cls, idx) in enumerate(lists):
        n = len(sc)
        cb[b, :n], cs[b, :n], cc[b, :n], ci[b, :n], cn[b] = box, sc, cls, idx, n
    cb, cs, cc, ci, cn = (t.to(DEV) for t in (cb, cs, cc, ci, cn))
    out = torch.full((B, MAX_DET, 6), -5.0, device=DEV)
    cnt = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    keep = torch.full((B + 1, MAX_DET), -4, dtype=torch.int32, device=DEV)  # one guard row behind
    ws = torch.zeros(int(_lib.lib.ydbl_nms_workspace(B, CAP, 30000)), dtype=torch.uint8, device=DEV)
    d = _lib.NmsDesc(cb.data_ptr(), cs.data_ptr(), cc.data_ptr(), ci.data_ptr(), cn.data_ptr(), B, CAP, 0.5, MAX_DET,
                     30000, int(agnostic), 7680.0, CLIP[1], CLIP[0], out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), 0,
                     0, int(per_image), keep.data_ptr() if with_idx else None)
    _lib.check(_lib.lib.ydbl_nms(C.byref(d), None), "ydbl_nms")
    torch.cuda.synchronize()
    return out.cpu(), cnt.cpu(), keep.cpu()


@pytest.mark.parametrize("multi", [False, True], ids=["single", "multi_label"])
@pytest.mark.parametrize("agnostic", [0, 1], ids=["classwise", "agnostic"])
@pytest.mark.parametrize("per_image", [0, 1], ids=["split", "per_image"])
def test_out_idx(per_image, agnostic, multi):
    lists = [make_list(64, 1 + multi, multi), make_list(600, 3 + multi, multi)]
    out0, cnt0, keep0 = run_nms(lists, per_image, agnostic, False)
    out1, cnt1, keep1 = run_nms(lists, per_image, agnostic, True)
    assert torch.equal(out0.view(torch.int32), out1.view(torch.int32)) and torch.equal(cnt0, cnt1)
    assert (keep0 == -4).all()  # NULL: nothing written
    assert (keep1[-1] == -4).all()  # the guard row
    for b, (box, sc, cls, idx) in enumerate(lists):
        n = int(cnt1[b])
        assert 0 < n < len(sc)  # the NMS kept some and dropped some
        assert (keep1[b, n:] == -1).all()
        pos = {int(v): j for j, v in enumerate(idx.tolist())}
        assert len(pos) == len(idx)
        rows = torch.tensor([pos[int(v)] for v in keep1[b, :n].tolist()])  # KeyError: not a candidate's index
        assert len(set(rows.tolist())) == n
        want = box[rows].clone()
        want[:, 0::2] = want[:, 0::2].clamp(0, CLIP[1])
        want[:, 1::2] = want[:, 1::2].clamp(0, CLIP[0])
        assert torch.equal(out1[b, :n, :4], want)
        assert torch.equal(out1[b, :n, 4], sc[rows]) and torch.equal(out1[b, :n, 5], cls[rows].float())
        if multi:  # the index carries the class: anchor * nc + cls
            assert torch.equal(keep1[b, :n] % NC, cls[rows])


def test_schedules_agree_on_out_idx():
    lists = [make_list(64, 1, False), make_list(600, 3, False)]
    a, b = run_nms(lists, 0, 0, True), run_nms(lists, 1, 0, True)
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
