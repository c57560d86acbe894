"""ydbl_gt_mask_bits, ydbl_mask_iou and ydbl_match_iou on the MI355X against the reference's expressions evaluated
by torch on the CPU (tests/segval_util.py), everything exact.

gt_mask_bits: index maps / planes of one batch of four images with 0, 1, 7 and 70 labels, resampled 4x
((24, 40) -> (96, 160), (16, 16) -> (64, 64)), copied ((96, 160) -> itself) and at a ratio that is no power of two
((17, 23) -> (96, 160), where the test first makes sure that no reference value is within 1e-5 of 0.5).
mask_iou: random and blob planes at 64 x 64, 96 x 160 and 75 x 150 (a tail word) for three images with 7, 0, 1
detections and 0, 3, 70 labels, with an empty, a full and two identical masks among them; 640 x 640 (6400 words, two
LDS chunks) with 2 detections x 3 labels; and 300 labels of one image (more than one label pass).
match_iou: against oracle.metrics.match_predictions on such IoU matrices with random classes and with single_cls;
the inputs are regenerated until no detection has two same-class labels at one IoU >= 0.5."""

import numpy as np
import pytest
import torch

import segval_util as SV
from oracle.metrics import IOUV, box_iou, match_predictions

pytestmark = pytest.mark.gpu
DEV = "cuda"
LABELS = (0, 1, 7, 70)


def _ofs(labels):
    return torch.tensor(np.concatenate([[0], np.cumsum(labels)]), dtype=torch.int32)


def _maps(seed, gh, gw):
    """One index map per image of LABELS: blocks of 3 x 2 pixels drawn from 0..nl, so that labels have area."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for nl in LABELS:
        coarse = torch.randint(0, nl + 1, ((gh + 2) // 3, (gw + 1) // 2), generator=g)
        out.append(coarse.repeat_interleave(3, 0).repeat_interleave(2, 1)[:gh, :gw].to(torch.uint8))
    return torch.stack(out)


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "planes"])
@pytest.mark.parametrize("ghw,hw", [((24, 40), (96, 160)), ((16, 16), (64, 64)), ((96, 160), (96, 160)),
                                    ((17, 23), (96, 160))], ids=["24x40_x4", "16x16_x4", "same", "17x23_odd"])
def test_gt_mask_bits(ghw, hw, overlap):
    from ydbl.utils.ops import gt_mask_bits

    maps = _maps(3, *ghw)
    if ghw == (17, 23):  # a condition on the inputs: the > 0.5 of the reference is not decided by rounding
        for m, nl in zip(maps, LABELS):
            if nl:
                v = SV.gt_planes_ref(m, nl, True, hw, values=True)
                assert ((v - 0.5).abs() > 1e-5).all()
    ofs = _ofs(LABELS)
    n_gt = int(ofs[-1])
    want = torch.cat([SV.gt_planes_ref(m, nl, True, hw) for m, nl in zip(maps, LABELS)]).to(torch.uint8)
    if overlap:
        src = maps
    else:  # the planes of the same labels; "set" is any nonzero byte
        src = torch.cat([(m[None] == torch.arange(1, nl + 1).view(nl, 1, 1)).to(torch.uint8) * (1 + 36 * (nl % 7))
                         for m, nl in zip(maps, LABELS)])
        assert src.shape[0] == n_gt and src.max() > 1
    bits, area = gt_mask_bits(src.to(DEV), ofs.to(DEV), n_gt, hw, overlap)
    torch.cuda.synchronize()
    assert bits.shape == (n_gt, hw[0], (hw[1] + 63) // 64) and bits.dtype == torch.int64
    assert np.array_equal(SV.words_np(bits), SV.pack_bits(want.numpy()))
    assert torch.equal(area.cpu(), want.view(n_gt, -1).sum(1).to(torch.int32))
    assert int(area.min()) >= 0 and int(area.max()) > 0
    again, area2 = gt_mask_bits(src.to(DEV), ofs.to(DEV), n_gt, hw, overlap)
    assert torch.equal(again, bits) and torch.equal(area2, area)


def _run_iou(det, counts, gt, labels, max_det):
    """det uint8 [n][count_b, H, W] and gt uint8 [n][nl_b, H, W] lists -> the kernel's (iou, inter, area_det) on the
    host and the per-image reference triples.  The detection planes sit compactly (row_offset = running count)."""
    from ydbl.utils.ops import mask_iou_bits, pack_mask_bits

    H, W = next(d for d in det + gt if len(d)).shape[1:]
    n = len(counts)
    offs = np.concatenate([[0], np.cumsum(counts)])
    dw = pack_mask_bits(torch.cat([torch.as_tensor(d).view(-1, H, W) for d in det]).to(DEV))
    gw = pack_mask_bits(torch.cat([torch.as_tensor(g).view(-1, H, W) for g in gt]).to(DEV))
    area_gt = torch.cat([torch.as_tensor(g).view(-1, H * W).sum(1) for g in gt]).to(torch.int32).to(DEV)
    row = torch.tensor(offs[:-1], dtype=torch.int64, device=DEV)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    ofs = _ofs(labels).to(DEV)
    iou, inter, area_det = mask_iou_bits(dw, row, cnt, max_det, gw, ofs, area_gt, (H, W), counts=True)
    only = mask_iou_bits(dw, row, cnt, max_det, gw, ofs, area_gt, (H, W))
    torch.cuda.synchronize()
    assert torch.equal(only, iou)  # the optional outputs change nothing
    refs = []
    for b in range(n):
        g, d = torch.as_tensor(gt[b]).view(-1, H * W), torch.as_tensor(det[b]).view(-1, H * W)
        refs.append((SV.mask_iou_ref(g.float(), d.float()), (g.long() @ d.long().T).to(torch.int32),
                     d.sum(1).to(torch.int32)))
    return iou.cpu(), inter.cpu(), area_det.cpu(), refs


def _check_iou(iou, inter, area_det, refs, counts, labels):
    g0 = 0
    for b, (k, nl) in enumerate(zip(counts, labels)):
        ri, rn, ra = refs[b]
        assert torch.equal(iou[g0:g0 + nl, :k], ri), b            # bit for bit
        assert torch.equal(inter[g0:g0 + nl, :k], rn), b
        assert torch.equal(area_det[b, :k], ra), b
        assert (iou[g0:g0 + nl, k:] == 0).all() and (inter[g0:g0 + nl, k:] == 0).all() and (area_det[b, k:] == 0).all()
        g0 += nl


@pytest.mark.parametrize("kind", ["random", "blob"])
@pytest.mark.parametrize("hw", [(64, 64), (96, 160), (75, 150)], ids=["64x64", "96x160", "75x150"])
def test_mask_iou(hw, kind):
    counts, labels = (7, 0, 1), (0, 3, 70)
    H, W = hw
    g = torch.Generator().manual_seed(H + W)

    def planes(k, seed):
        if kind == "blob":
            return torch.from_numpy(SV.blob_planes(k, H, W, seed))
        return (torch.rand(k, H, W, generator=g) > 0.6).to(torch.uint8)

    det = [planes(k, 10 + b) for b, k in enumerate(counts)]
    gt = [planes(nl, 20 + b) for b, nl in enumerate(labels)]
    det[0][0], det[0][1], det[0][3] = 0, 1, det[0][2]  # an empty, a full and two identical masks
    gt[2][0], gt[2][1], gt[2][2], gt[2][4] = 0, 1, det[2][0], gt[2][3]
    gt[1][0] = 1  # (an image without detections: only its zero columns)
    iou, inter, area_det, refs = _run_iou(det, counts, gt, labels, max_det=9)
    _check_iou(iou, inter, area_det, refs, counts, labels)
    assert iou[3 + 2, 0] == refs[2][0][2, 0] and refs[2][0][2, 0] > 0.99  # identical masks
    assert iou[3 + 0, 0] == 0 and 0 < iou[3 + 1, 0] <= 1


def test_mask_iou_640_crosses_the_lds_chunk():
    det = [torch.from_numpy(SV.blob_planes(2, 640, 640, 1))]
    gt = [torch.from_numpy(SV.blob_planes(3, 640, 640, 2))]
    gt[0][2] = det[0][1]
    gt[0][2][600:, :] = 1  # differs from the detection in the second chunk only (rows >= 410)
    iou, inter, area_det, refs = _run_iou(det, (2,), gt, (3,), max_det=3)
    _check_iou(iou, inter, area_det, refs, (2,), (3,))
    assert 0 < iou[2, 1] < 1


def test_mask_iou_300_labels_take_two_passes():
    g = torch.Generator().manual_seed(9)
    det = [(torch.rand(5, 64, 64, generator=g) > 0.5).to(torch.uint8)]
    gt = [(torch.rand(300, 64, 64, generator=g) > 0.5).to(torch.uint8)]
    iou, inter, area_det, refs = _run_iou(det, (5,), gt, (300,), max_det=6)
    _check_iou(iou, inter, area_det, refs, (5,), (300,))


def _match_case(seed, counts, labels, hw=(64, 64), nc=3):
    """Blob detections, labels that are shifted copies of them (so that IoUs spread over the thresholds) or blobs of
    their own, random classes.  -> (det [n, max_det, 6], per-image reference IoU matrices, gt_cls list)."""
    rng = np.random.default_rng(seed)
    H, W = hw
    dets, gts, ious = [], [], []
    for b, (k, nl) in enumerate(zip(counts, labels)):
        d = SV.blob_planes(k, H, W, seed * 10 + b)
        g = SV.blob_planes(nl, H, W, seed * 10 + 5 + b)
        for l in range(min(k, nl)):
            g[l] = np.roll(d[l], int(rng.integers(0, 6)), axis=1)
        dets.append(torch.from_numpy(d))
        gts.append(torch.from_numpy(g))
        ious.append(SV.mask_iou_ref(gts[-1].view(-1, H * W).float(), dets[-1].view(-1, H * W).float()))
    max_det = max(counts) + 2
    det = torch.zeros(len(counts), max_det, 6)
    det[..., 5] = torch.from_numpy(rng.integers(0, nc, (len(counts), max_det)).astype(np.float32))
    det[..., 4] = torch.from_numpy(np.sort(rng.random((len(counts), max_det)).astype(np.float32))[:, ::-1].copy())
    gt_cls = [torch.from_numpy(rng.integers(0, nc, nl).astype(np.float32)) for nl in labels]
    for b, (k, nl) in enumerate(zip(counts, labels)):  # most shifted copies carry their detection's class
        for l in range(min(k, nl)):
            if rng.random() < 0.8:
                gt_cls[b][l] = det[b, l, 5]
    return det, ious, gt_cls


@pytest.mark.parametrize("single_cls", [False, True], ids=["classes", "single_cls"])
def test_match_iou_against_the_oracle(single_cls):
    from ydbl.engine.validator import match_iou_batch

    counts, labels = (7, 0, 5, 3), (4, 3, 9, 0)
    for seed in range(1, 50):  # regenerate until the inputs have no exact tie (a condition on the inputs)
        det, ious, gt_cls = _match_case(seed, counts, labels)
        pcs = [torch.zeros(k) if single_cls else det[b, :k, 5] for b, k in enumerate(counts)]
        if not any(SV.has_tie(i, c, p) for i, c, p in zip(ious, gt_cls, pcs)):
            break
    else:
        raise AssertionError("no tie-free case found")
    n_gt, max_det = sum(labels), det.shape[1]
    iou = torch.full((n_gt, max_det), float("nan"))
    g0 = 0
    for b, (k, nl) in enumerate(zip(counts, labels)):
        iou[g0:g0 + nl, :k] = ious[b]
        iou[g0:g0 + nl, k:] = 0
        g0 += nl
    got = match_iou_batch(det.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), iou.to(DEV),
                          torch.cat(gt_cls).to(DEV), _ofs(labels).to(DEV), IOUV, single_cls).cpu()
    assert got.shape == (len(counts), max_det, 10)
    some = 0
    for b, (k, nl) in enumerate(zip(counts, labels)):
        want = match_predictions(pcs[b], gt_cls[b], ious[b], IOUV) if nl and k else torch.zeros(k, 10, dtype=torch.bool)
        assert torch.equal(got[b, :k], want), b
        assert not got[b, k:].any()
        some += int(want.sum())
    assert some > 0 and some < sum(counts) * 10


def test_match_predictions_on_boxes_is_unchanged():
    from ydbl.engine.validator import match_batch

    g = torch.Generator().manual_seed(4)
    counts = (6, 0, 3)
    det = torch.zeros(3, 8, 6)
    xy = torch.rand(3, 8, 2, generator=g) * 60
    det[..., :2], det[..., 2:4] = xy, xy + 10 + torch.rand(3, 8, 2, generator=g) * 30
    det[..., 4] = torch.rand(3, 8, generator=g)
    det[..., 5] = torch.randint(0, 2, (3, 8), generator=g).float()
    gt_box = torch.cat([det[0, :4, :4] + torch.rand(4, 4, generator=g) * 4, det[2, :2, :4] + 1.5,
                        torch.tensor([[5.0, 5.0, 20.0, 20.0]])])
    gt_cls = torch.cat([det[0, :4, 5], det[2, :2, 5], torch.tensor([1.0])])
    bidx = torch.tensor([0, 0, 0, 0, 2, 2, 1])
    got = match_batch(det.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), gt_box, gt_cls, bidx).cpu()
    for b, k in enumerate(counts):
        sel = bidx == b
        want = match_predictions(det[b, :k, 5], gt_cls[sel], box_iou(gt_box[sel], det[b, :k, :4]), IOUV)
        assert torch.equal(got[b, :k], want) and not got[b, k:].any()
    assert got.any()


def test_mask_iou_entry_point():
    """ydbl.utils.metrics.mask_iou on CUDA tensors: the reference's values for 0 / 1 masks."""
    from ydbl.utils.metrics import mask_iou

    g = torch.Generator().manual_seed(2)
    a, b = (torch.rand(5, 1000, generator=g) > 0.5).float(), (torch.rand(8, 1000, generator=g) > 0.4).float()
    got = mask_iou(a.to(DEV), b.to(DEV))
    assert got.shape == (5, 8) and torch.equal(got.cpu(), SV.mask_iou_ref(a, b))
    assert mask_iou(a[:0].to(DEV), b.to(DEV)).shape == (0, 8)
