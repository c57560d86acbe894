"""ydbl_deconv2x2_nhwc on the MI355X: ConvTranspose2d(c, c, 2, 2, 0) on NHWC views against fp64 conv_transpose2d.

Bound (a2c2f_util.leg_bound): twice the torch-CPU leg of the same precision's distance to fp64 plus one rounding of
max|y|.  The map is 5 x 7 with n = 2: 70 pixels, neither a multiple of the 16-pixel MFMA tile nor of a workgroup's
pixels, and more than one workgroup.  A second case gives x and y a padded channel stride and checks that the pad lanes
keep their fill."""

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from a2c2f_util import leg_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, H, W = 2, 5, 7
FILL = -77.0


def make(c, bias, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, c, H, W, generator=g)
    w = torch.randn(c, c, 2, 2, generator=g) / c**0.5
    b = torch.randn(c, generator=g) if bias else None
    return x, w, b


def run(x, w, b, half, pad=0, act=0):
    """The kernel on NCHW x, torch-layout w -> (y NCHW fp32 on the host, the raw x / y buffers [pixels, cs])."""
    from ydbl import _lib

    dt = torch.float16 if half else torch.float32
    n, c, h, wd = x.shape
    co = w.shape[1]
    cs_x, cs_y = c + pad, co + pad
    xb = torch.full((n * h * wd, cs_x), FILL, dtype=dt, device=DEV)
    xb[:, :c] = x.permute(0, 2, 3, 1).reshape(-1, c).to(DEV, dt)
    x0 = xb.clone()
    yb = torch.full((n * 2 * h * 2 * wd, cs_y), FILL, dtype=dt, device=DEV)
    wp = w.permute(2, 3, 1, 0).contiguous().to(DEV, dt)
    bd = b.to(DEV) if b is not None else None
    d = _lib.DeconvDesc(_lib.View(xb.data_ptr(), n, h, wd, c, cs_x, _lib.dtype_code(dt)),
                        _lib.View(yb.data_ptr(), n, 2 * h, 2 * wd, co, cs_y, _lib.dtype_code(dt)), wp.data_ptr(),
                        bd.data_ptr() if bd is not None else None, act)
    _lib.check(_lib.lib.ydbl_deconv2x2_nhwc(C.byref(d), None), "ydbl_deconv2x2_nhwc")
    torch.cuda.synchronize()
    assert torch.equal(xb, x0)  # the input is only read
    y = yb[:, :co].reshape(n, 2 * h, 2 * wd, co).permute(0, 3, 1, 2).float().cpu()
    return y, yb.cpu()


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("c", [32, 64, 96])
def test_deconv_against_fp64(c, half, bias):
    x, w, b = make(c, bias, 10 * c + bias)
    if half:  # the operands the half leg and the kernel both see
        x, w = x.half().float(), w.half().float()
    y64 = F.conv_transpose2d(x.double(), w.double(), b.double() if bias else None, stride=2)
    if half:
        leg = F.conv_transpose2d(x.half(), w.half(), b.half() if bias else None, stride=2)
    else:
        leg = F.conv_transpose2d(x, w, b, stride=2)
    y, _ = run(x, w, b, half)
    err = (y.double() - y64).abs().max().item()
    bound = leg_bound(leg, y64, half)
    print(f"deconv2x2 c={c} {'half' if half else 'fp32'} bias={bias}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
def test_padded_channel_stride_leaves_the_pad_lanes(half):
    c, pad = 64, 8
    x, w, b = make(c, True, 5)
    y_dense, _ = run(x, w, b, half)
    y_pad, raw = run(x, w, b, half, pad=pad)
    assert torch.equal(y_dense, y_pad)  # the same values whatever the pitch
    assert (raw[:, c:].float() == FILL).all()


def test_activation_and_refusals():
    from ydbl import _lib

    x, w, b = make(32, True, 9)
    y64 = F.silu(F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2))
    leg = F.silu(F.conv_transpose2d(x, w, b, stride=2))
    y, _ = run(x, w, b, False, act=_lib.ACT_SILU)
    assert (y.double() - y64).abs().max().item() <= leg_bound(leg, y64, False)
    with pytest.raises(_lib.YdblError, match="multiples of 32"):
        run(*make(48, True, 1), False)
