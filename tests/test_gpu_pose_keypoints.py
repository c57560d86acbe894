"""ydbl_pose_keypoints alone on the MI355X, at the smallest case that can still go wrong: three levels of 8 x 8, 4 x 4
and 2 x 2 cells (strides 8 / 16 / 32, 84 anchors), three images with 0, 3 and 8 live slots of max_det = 8, keep_idx
hitting the first and last anchor of every level, one index past the levels, the multi-label index form (nc = 3), level
views whose channel stride (56) is wider than their 51 channels, f16 and f32 maps, kpt_shape (17, 3) and (5, 2).

x / y must EQUAL torch's fp32 evaluation of the reference formula on the stored values (v * 2 and * stride are exact:
one rounding); the visibility lies within the project's fp32 elementwise bound (rtol = atol = 1e-5,
tests/test_gpu_ops.py) of the fp64 sigmoid; every slot at or past its count is zero; two launches give the same bytes."""

import ctypes as C

import pytest
import torch

import pose_util as P

pytestmark = pytest.mark.gpu

HWS = [(8, 8), (4, 4), (2, 2)]
STRIDES = [8.0, 16.0, 32.0]
A = 84
N, MAX_DET = 3, 8
COUNTS = [0, 3, 8]
# image 1: first anchor, last anchor of level 0, first of level 1; image 2: the level ends and starts, and one past
ANCHORS = [[5, 6, 7, 8, 9, 10, 11, 12], [0, 63, 64, 70, 71, 72, 73, 74], [79, 80, 83, 84, 0, 63, 17, 42]]


def maps(kpt_shape, cs, dtype, seed):
    """Per level an NHWC buffer [N, h, w, cs] of N(0, 2) values in `dtype` (the lanes past nk hold garbage the kernel
    must not read as keypoints), and the raw [N, A, nk] values as stored."""
    nk = kpt_shape[0] * kpt_shape[1]
    g = torch.Generator().manual_seed(seed)
    bufs = [(torch.randn(N, h, w, cs, generator=g) * 2).to(dtype) for h, w in HWS]
    raw = torch.cat([b[..., :nk].reshape(N, -1, nk) for b in bufs], 1)
    return bufs, raw


def launch(bufs, kpt_shape, keep, count, nc):
    from ydbl import _lib

    K, ndim = kpt_shape
    dev = [b.cuda() for b in bufs]
    views = (_lib.View * 3)(*[_lib.View(b.data_ptr(), N, h, w, K * ndim, b.shape[-1], _lib.dtype_code(b.dtype))
                              for b, (h, w) in zip(dev, HWS)])
    keep_d, count_d = keep.cuda(), count.cuda()
    out = torch.full((N, MAX_DET, K, ndim), float("nan"), device="cuda")
    d = _lib.PoseKptDesc(views, 3, nc, (C.c_float * 3)(*STRIDES), keep_d.data_ptr(), count_d.data_ptr(), N, MAX_DET,
                         K, ndim, out.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib.ydbl_pose_keypoints(d, stream), "ydbl_pose_keypoints")
    first = out.clone()
    out.fill_(float("nan"))
    _lib.check(_lib.lib.ydbl_pose_keypoints(d, stream), "ydbl_pose_keypoints")
    torch.cuda.synchronize()
    return first.cpu(), out.cpu()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("kpt_shape,cs", [((17, 3), 56), ((5, 2), 16)], ids=["17x3", "5x2"])
@pytest.mark.parametrize("nc", [0, 3], ids=["anchor", "multilabel"])
def test_keypoints_kernel(kpt_shape, cs, dtype, nc):
    K, ndim = kpt_shape
    bufs, raw = maps(kpt_shape, cs, dtype, seed=K + ndim)
    anchors = torch.tensor(ANCHORS)
    # the multi-label index anchor * nc + cls, every class occurring
    keep = (anchors * nc + torch.arange(MAX_DET)[None] % nc if nc else anchors).to(torch.int32)
    count = torch.tensor(COUNTS, dtype=torch.int32)
    got, again = launch(bufs, kpt_shape, keep, count, nc)
    assert torch.equal(got, again) and not torch.isnan(got).any()
    for b in range(N):
        k = COUNTS[b]
        assert (got[b, k:] == 0).all()
        for j in range(k):
            a = int(anchors[b, j])
            if a >= A:  # past the levels: a zero row
                assert (got[b, j] == 0).all()
                continue
            want = P.decode_rows(raw[b, a][None], [a], HWS, STRIDES, ndim)[0]
            assert torch.equal(got[b, j, :, :2], want[:, :2]), (b, j, a)
            if ndim == 3:
                v64 = raw[b, a].double().reshape(K, 3)[:, 2].sigmoid()
                assert torch.allclose(got[b, j, :, 2].double(), v64, rtol=1e-5, atol=1e-5)
    assert (got[2, :3] != 0).any() and (got[1, :3] != 0).any()  # live rows hold values
