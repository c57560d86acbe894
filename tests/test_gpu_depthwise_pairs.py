"""The depthwise inner loops (channel-pair packed fp32 FMAs) pinned to a CPU restatement, bit for bit.

ydbl_dsconv_nhwc is driven with an identity pointwise matrix, zero biases and no activation, so its fp16 output
is exactly the fp16-rounded depthwise value: one 1.0 * v term per MFMA row, every other term 0, all exact in fp32.
The restatement is a numpy fp32 loop, acc = float32(acc + x * w) in (ky, kx) order.  x and w hold fp16 values, so
each product is exact in fp32 and a fused multiply-add equals multiply-then-add: the loop is exact on any hardware,
and the lean and the chunked kernel, which otherwise only check each other, both have to land on it.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _plan():
    from ydbl.runtime import Plan

    return Plan(torch.device(DEV), torch.float16)


def _upload(plan, x):
    n, c, h, w = x.shape
    v = plan.alloc(n, h, w, c)
    v.torch().copy_(x.permute(0, 2, 3, 1).to(torch.float16))
    return v


def _run(plan):
    plan.run()
    torch.cuda.synchronize()


def _f16_valued(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().float()


def _dw_restated(x, w, k, s, pad, dil):
    """x [n, c, h, w], w [c, k, k], fp32 arrays of fp16 values -> fp16 [n, c, ho, wo]; fp32 accumulation in
    (ky, kx) order, one rounding per term.  Padded taps add an exact zero, as skipping them does."""
    n, c, h, wd = x.shape
    ho, wo = (h + 2 * pad - dil * (k - 1) - 1) // s + 1, (wd + 2 * pad - dil * (k - 1) - 1) // s + 1
    xp = np.zeros((n, c, h + 2 * pad, wd + 2 * pad), np.float32)
    xp[:, :, pad:pad + h, pad:pad + wd] = x
    acc = np.zeros((n, c, ho, wo), np.float32)
    for ky in range(k):
        for kx in range(k):
            win = xp[:, :, ky * dil:ky * dil + (ho - 1) * s + 1:s, kx * dil:kx * dil + (wo - 1) * s + 1:s]
            prod = (win * w[None, :, ky, kx, None, None]).astype(np.float32)  # exact: 11-bit x 11-bit significands
            acc = (acc + prod).astype(np.float32)
    return acc.astype(np.float16)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int16)


# (channels, k, stride, YDBL_DS_LEAN, kernel the route lands on)
DS_CASES = [
    (64, 3, 1, None, "lean 64"), (64, 7, 1, None, "lean 64"), (128, 7, 1, None, "lean 128, 512 threads"),
    (128, 3, 2, None, "lean 128 stride 2"), (32, 3, 1, None, "chunked"), (128, 3, 2, "0", "chunked"),
    (64, 7, 1, "0", "chunked"),
]


@pytest.mark.parametrize("shape", [(2, 9, 13), (1, 16, 16)])
@pytest.mark.parametrize("c,k,s,lean,route", DS_CASES)
def test_dsconv_depthwise_matches_restatement(c, k, s, lean, route, shape, monkeypatch):
    import torch.nn as nn

    from ydbl import _lib
    from ydbl.nn import modules as M

    if lean is None:
        monkeypatch.delenv("YDBL_DS_LEAN", raising=False)
    else:
        monkeypatch.setenv("YDBL_DS_LEAN", lean)
    n, h, w = shape
    x = _f16_valued(n, c, h, w, seed=c + k + h)
    wt = _f16_valued(c, 1, k, k, seed=7 * c + k, scale=0.3)
    dw = nn.Conv2d(c, c, k, s, k // 2, groups=c, bias=False)
    with torch.no_grad():
        dw.weight.copy_(wt)
    plan = _plan()
    y = M.emit_dsconv(plan, dw, _upload(plan, x), None, torch.eye(c).reshape(c, c, 1, 1), torch.zeros(c),
                      act=_lib.ACT_NONE)
    assert [st.fn.__name__ for st in plan.steps] == ["ydbl_dsconv_nhwc"]
    _run(plan)
    got = y.nchw().cpu().numpy()
    want = _dw_restated(x.numpy(), wt.numpy()[:, 0], k, s, k // 2, 1)
    assert got.dtype == np.float16 and got.shape == want.shape
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (route, int(bad.sum()), float(np.abs(got.astype(np.float32) - want.astype(np.float32)).max()))


def test_dw_pair_matches_restatement():
    """dw_pair_kernel: 5x5, then 7x7 dilation 3 on the fp16-rounded first output, 16 channels at 20x20."""
    import torch.nn as nn

    from ydbl.nn import modules as M

    c, h, w = 16, 20, 20
    x = _f16_valued(2, c, h, w, seed=5)
    w0 = _f16_valued(c, 1, 5, 5, seed=6, scale=0.3)
    w1 = _f16_valued(c, 1, 7, 7, seed=7, scale=0.3)
    c0 = nn.Conv2d(c, c, 5, padding=2, groups=c, bias=False)
    c1 = nn.Conv2d(c, c, 7, padding=9, groups=c, dilation=3, bias=False)
    with torch.no_grad():
        c0.weight.copy_(w0)
        c1.weight.copy_(w1)
    plan = _plan()
    a1, a2 = M.emit_dw_pair(plan, c0, c1, _upload(plan, x))
    _run(plan)
    want1 = _dw_restated(x.numpy(), w0.numpy()[:, 0], 5, 1, 2, 1)
    want2 = _dw_restated(want1.astype(np.float32), w1.numpy()[:, 0], 7, 1, 9, 3)
    assert np.array_equal(_bits(a1.nchw().cpu().numpy()), _bits(want1))
    assert np.array_equal(_bits(a2.nchw().cpu().numpy()), _bits(want2))


@pytest.mark.parametrize("k,s,dil", [(3, 1, 1), (3, 2, 1), (7, 1, 3)])
def test_dwconv_lds_matches_restatement(k, s, dil):
    """dwconv_lds_kernel through ydbl_dwconv2d_nhwc: 64 channels, a ragged 9x13 map."""
    import torch.nn as nn

    from ydbl.nn import modules as M

    c = 64
    x = _f16_valued(2, c, 9, 13, seed=11 + k)
    wt = _f16_valued(c, 1, k, k, seed=12 + k, scale=0.3)
    pad = dil * (k - 1) // 2
    conv = nn.Conv2d(c, c, k, s, pad, dilation=dil, groups=c, bias=False)
    with torch.no_grad():
        conv.weight.copy_(wt)
    plan = _plan()
    y = M.emit_conv2d(plan, conv, _upload(plan, x), None)
    _run(plan)
    want = _dw_restated(x.numpy(), wt.numpy()[:, 0], k, s, pad, dil)
    assert np.array_equal(_bits(y.nchw().cpu().numpy()), _bits(want))
