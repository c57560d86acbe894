"""ydbl_kpt_oks and the matching on the MI355X: three images with 0, 1 and 7 labels against 0, 3 and 8 live slots of
max_det = 8; K = 17 with OKS_SIGMA and K = 5 with the uniform sigma.  Among the labels one has no visible keypoint (its
OKS row is 0), one a zero-area box, and one's prediction is an exact copy (OKS = visible / (visible + 1e-7)).

OKS is compared against the restated kpt_iou in fp64 at rtol = atol = 1e-5: a term's error is bounded by
e * exp(-e) <= 0.37 times a handful of fp32 roundings (the difference, two squares, a sum, three products, a quotient,
expf: ~10 * 2^-24 = 6e-7), an order below the bound, and the mean of <= 17 such terms is no worse.  ydbl_match_iou on
the device's matrix must give `correct` EQUAL to the restated match_predictions on the same matrix.  The inputs come
from a fixed seed, chosen on the CPU so that on the fp64 matrix no same-class pair lies within 1e-4 of any of the ten
thresholds: asserted first as a precondition, no pair is excluded."""

import numpy as np
import pytest
import torch

import pose_util as P
from oracle.metrics import IOUV, match_predictions

N, MAX_DET = 3, 8
COUNTS = [0, 3, 8]
LABELS = [0, 1, 7]
SEEDS = {17: 1, 5: 1}  # per K: the seed the threshold precondition holds for (checked below)


def sigma_of(K):
    return P.OKS_SIGMA if K == 17 else np.ones(K) / K


def case(K, ndim, seed):
    """Labels and predictions in a 128 x 128 frame.  Label l of an image is shadowed by detection slot l (when live)
    at a noise level that grows with l, so the OKS values spread over (0, 1]; the other slots are far away."""
    g = torch.Generator().manual_seed(seed)
    n_gt = sum(LABELS)
    bidx = torch.tensor([b for b, k in enumerate(LABELS) for _ in range(k)])
    xy = torch.rand(n_gt, 2, generator=g) * 60 + 10
    wh = torch.rand(n_gt, 2, generator=g) * 40 + 20
    gt_box = torch.cat([xy, xy + wh], 1)
    gt_kpts = torch.cat([xy[:, None] + torch.rand(n_gt, K, 2, generator=g) * wh[:, None],
                         torch.randint(0, 3, (n_gt, K, 1), generator=g).float()], -1)
    gt_kpts[0, 0, 2] = 2.0  # the single label of image 1 has a visible point
    gt_kpts[3, :, 2] = 0.0  # (image 2's third label) no visible keypoint: OKS row 0
    gt_box[4, 2:] = gt_box[4, :2]  # zero-area box
    gt_kpts[1, 1, 2] = 1.0  # image 2's first label, whose slot is an exact copy, has a visible point
    gt_cls = torch.randint(0, 2, (n_gt,), generator=g).float()
    pred = torch.rand(N, MAX_DET, K, ndim, generator=g) * 128
    det = torch.zeros(N, MAX_DET, 6)
    det[..., 4] = torch.rand(N, MAX_DET, generator=g)
    det[..., 5] = torch.randint(0, 2, (N, MAX_DET), generator=g).float()
    sig = torch.tensor(sigma_of(K), dtype=torch.float32)
    ofs = [0, *np.cumsum(LABELS).tolist()]
    for b in range(N):
        for l in range(LABELS[b]):
            if l >= COUNTS[b]:
                continue
            gi = ofs[b] + l
            scale = (wh[gi].prod() * 0.53).sqrt() * sig[:, None] * (0.3 * l)
            pred[b, l, :, :2] = gt_kpts[gi, :, :2] + torch.randn(K, 2, generator=g) * scale
            det[b, l, 5] = gt_cls[gi]
    for b in range(N):  # slots past the count hold garbage the kernel must not read into a result
        pred[b, COUNTS[b]:] = 1e30
    return pred, det, gt_kpts, gt_box, gt_cls, bidx


def oks64(K, ndim, seed):
    pred, det, gt_kpts, gt_box, gt_cls, bidx = case(K, ndim, seed)
    return P.oks_ref(pred, COUNTS, gt_kpts, gt_box, bidx, sigma_of(K), torch.float64)


@pytest.mark.parametrize("K,ndim", [(17, 3), (5, 2)], ids=["17x3", "5x2"])
def test_threshold_precondition(K, ndim):
    """(CPU) the seed keeps every same-class pair's fp64 OKS at least 1e-4 from every threshold."""
    pred, det, gt_kpts, gt_box, gt_cls, bidx = case(K, ndim, SEEDS[K])
    ref = oks64(K, ndim, SEEDS[K])
    assert [si for si, _ in ref] == [1, 2]
    assert P.threshold_margin(ref, gt_cls, bidx, det, COUNTS) >= 1e-4
    big = ref[1][1]
    assert (big[2] == 0).all()  # label 3 (the image's third): no visible point
    nv = float((gt_kpts[1, :, 2] != 0).sum())
    # the exact copy (noise level 0): visible / (visible + 1e-7), whose denominator torch forms in fp32 (int + float)
    assert nv >= 1 and big[0, 0].item() == pytest.approx(nv / (nv + 1e-7), abs=1e-7)
    assert ((big > 0.3) & (big < 0.99)).sum() >= 3  # values the thresholds separate


@pytest.mark.gpu
@pytest.mark.parametrize("K,ndim", [(17, 3), (5, 2)], ids=["17x3", "5x2"])
def test_oks_and_matching(K, ndim):
    from ydbl.engine.validator import group_labels, match_iou_batch
    from ydbl.utils.ops import kpt_oks

    pred, det, gt_kpts, gt_box, gt_cls, bidx = case(K, ndim, SEEDS[K])
    ref = oks64(K, ndim, SEEDS[K])
    assert P.threshold_margin(ref, gt_cls, bidx, det, COUNTS) >= 1e-4
    dev = torch.device("cuda")
    count = torch.tensor(COUNTS, dtype=torch.int32, device=dev)
    boxes, cls, ofs, n_gt = group_labels(gt_box, gt_cls, bidx, N, dev)
    sigma = torch.tensor(sigma_of(K), dtype=torch.float32, device=dev)
    oks = kpt_oks(pred.to(dev).contiguous(), count, gt_kpts.to(dev).contiguous(), boxes, ofs, sigma)
    again = kpt_oks(pred.to(dev).contiguous(), count, gt_kpts.to(dev).contiguous(), boxes, ofs, sigma)
    correct = match_iou_batch(det.to(dev), count, oks, cls, ofs, IOUV)
    torch.cuda.synchronize()
    oks, correct = oks.cpu(), correct.cpu()
    assert oks.shape == (sum(LABELS), MAX_DET) and torch.equal(oks, again.cpu()) and torch.isfinite(oks).all()
    o = [0, *np.cumsum(LABELS).tolist()]
    for b in range(N):  # columns at or past the count are 0
        assert (oks[o[b]:o[b + 1], COUNTS[b]:] == 0).all()
    for si, r64 in ref:
        got = oks[o[si]:o[si + 1], :COUNTS[si]].double()
        assert torch.allclose(got, r64, rtol=1e-5, atol=1e-5), (si, (got - r64).abs().max())
        want = match_predictions(det[si, :COUNTS[si], 5], gt_cls[bidx == si], oks[o[si]:o[si + 1], :COUNTS[si]], IOUV)
        assert torch.equal(correct[si, :COUNTS[si]], want) and not correct[si, COUNTS[si]:].any()
        assert torch.equal(want, match_predictions(det[si, :COUNTS[si], 5], gt_cls[bidx == si], r64.float(), IOUV))
    assert not correct[0].any() and correct[2].any()
    assert (oks[3] == 0).all()  # the label without a visible keypoint
    assert oks[1, 0].item() == pytest.approx(1.0, abs=1e-6)  # the exact copy
