"""ydbl_global_avgpool alone, through the C-ABI, on the MI355X: values against the fp64 mean of the same view under
the derived bound (embed_util.pool_bound), the output row stride, determinism (run to run, and an image pooled
alone against the same image inside a batch), graph capture.

Inputs are seeded randn + 3 laid into a wider buffer, so every view is a true channel slice; each case runs in fp16
and fp32.  (c 20, offset 4) breaks the 16-byte rule in fp16 only -- 4 floats are 16 bytes -- so (c 20, cs 27,
offset 3) takes the scalar path in fp32 too."""

import ctypes as C

import pytest
import torch

from embed_util import pool_bound

pytestmark = pytest.mark.gpu

# n, h, w, c, cs, slice offset
CASES = [
    (1, 1, 1, 8, 8, 0),       # degenerate map
    (3, 5, 7, 24, 64, 8),     # ragged pixel tail, strided slice
    (2, 3, 4, 256, 256, 0),   # the default layer's shape at 96 x 128
    (2, 9, 5, 20, 24, 4),     # breaks the 16-byte rule (fp16): the scalar path
    (2, 9, 5, 20, 27, 3),     # ... and in fp32: odd channel stride, odd offset
    (3, 80, 80, 16, 16, 0),   # many pixel chunks per image (the partials path)
    (5, 48, 64, 16, 32, 16),  # chunked, strided: the batch-independence case
    (2, 20, 20, 300, 304, 0),  # more than 256 scalar channels / a ragged vector count, several chunks
]
DTYPES = [torch.float16, torch.float32]


def make_view(n, h, w, c, cs, off, dtype, seed=0):
    """(TV of the slice, the buffer): element (n, y, x, ch) of the view at buf[off + ((n*h + y)*w + x)*cs + ch]."""
    from ydbl.runtime import TV

    g = torch.Generator().manual_seed(seed + 1000 * c + h * w)
    buf = (torch.randn(n * h * w * cs + off, generator=g) + 3.0).to(dtype).cuda()
    return TV(buf, off, n, h, w, c, cs), buf


def pool(v, out=None, col=0, stream=None):
    """Run the kernel on view v into out[:, col:col+c] (a fresh [n, c] tensor by default); returns out."""
    from ydbl import _lib

    if out is None:
        out = torch.full((v.n, v.c), -7.0, dtype=v.dtype, device="cuda")
    d = _lib.AvgPoolDesc(v.struct(), out.data_ptr() + col * out.element_size(), out.stride(0), None, 0)
    need = int(_lib.lib.ydbl_global_avgpool_workspace(d))
    assert need >= 0
    ws = torch.empty(max(need, 4), dtype=torch.uint8, device="cuda")
    if need:
        d.workspace, d.workspace_bytes = ws.data_ptr(), need
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _lib.check(_lib.lib.ydbl_global_avgpool(d, C.c_void_p(s)), "ydbl_global_avgpool")
    pool.keep = (d, ws)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n{}_{}x{}_c{}_cs{}_o{}".format(*c))
def test_value_within_derived_bound(case, dtype):
    n, h, w, c, cs, off = case
    v, _ = make_view(n, h, w, c, cs, off, dtype)
    got = pool(v)
    torch.cuda.synchronize()
    x = v.torch().cpu()
    ref = x.double().mean((1, 2))
    bound = pool_bound(x, dtype == torch.float16)
    err = (got.cpu().double() - ref).abs()
    print(f"avgpool {case} {dtype}: max err / bound = {(err / bound).max().item():.3f}")
    assert got.dtype == dtype and got.shape == (n, c)
    assert (err <= bound).all(), (err / bound).max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=["vec", "scalar", "chunked"])
def test_output_row_stride_leaves_the_rest_untouched(case, dtype):
    n, h, w, c, cs, off = case
    v, _ = make_view(n, h, w, c, cs, off, dtype)
    wide = torch.full((n, c + 11), -7.0, dtype=dtype, device="cuda")
    pool(v, wide, col=5)
    dense = pool(v)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, 5:5 + c], dense)
    assert (wide[:, :5] == -7.0).all() and (wide[:, 5 + c:] == -7.0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n{}_{}x{}_c{}_cs{}_o{}".format(*c))
def test_two_runs_bit_equal(case, dtype):
    v, _ = make_view(*case, dtype)
    a, b = pool(v), pool(v)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", [CASES[6], CASES[5], CASES[7]], ids=["48x64", "80x80", "20x20c300"])
def test_image_alone_equals_image_in_batch(case, dtype):
    from ydbl.runtime import TV

    n, h, w, c, cs, off = case
    v, buf = make_view(n, h, w, c, cs, off, dtype)
    batch = pool(v)
    for i in (0, n - 1):
        one = TV(buf, off + i * h * w * cs, 1, h, w, c, cs)
        alone = pool(one)
        torch.cuda.synchronize()
        assert torch.equal(alone[0], batch[i]), i


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "fp32"])
@pytest.mark.parametrize("case", [CASES[1], CASES[6]], ids=["one_launch", "two_launches"])
def test_graph_capture_replays_bit_equal(case, dtype):
    v, _ = make_view(*case, dtype)
    eager = pool(v).clone()
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pool(v, out)
    keep = pool.keep  # the descriptor's workspace outlives the capture
    for _ in range(2):
        out.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
    del keep
