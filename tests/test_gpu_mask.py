"""ydbl_process_mask on the MI355X against the fp64 restatement of process_mask / process_mask_native
(tests/seg_util.py).

The rule (seg_util.mask_check): with v64 the restatement's fp64 value before the final `> 0` and S the same pipeline on
|coef|, |proto|, a pixel with S == 0 must be exactly 0; elsewhere the mask must equal v64 > 0 unless |v64| <= 2^-16 S
(the near-zero set, whose sign fp32 arithmetic cannot be held to), and that set may hold at most 0.1 % of the S > 0
pixels (tests/test_seg_host.py checks the same on the CPU legs).  The kernel's own fp32 error is a few 2^-24 S per
term, far inside 2^-16 S.

Shapes: prototypes [2, 24, 40, nm] and [2, 16, 16, nm]; outputs 96 x 160 and 64 x 64 (upsample=True: 3 x 3 and 2 x 1
tiles of 32 x 64), the grid itself (upsample=False: one partial tile), and 75 x 150, 101 x 127, 200 x 173 through
scale_masks' window (odd row lengths: rows that are not 16-byte aligned take the single stores).  Every launch writes
into a buffer with max_det planes per image and a guard band on both sides: planes past an image's count and the
bands must keep their fill."""


import pytest
import torch

import seg_util as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_DET = 9
FILL = 7
LEVELS = [(6, 10), (3, 5), (2, 3)]


def run(form, proto, boxes, counts, frame, coef=None, levels=None, keep=None, nc=0, u8=False, proto_pad=0):
    """One launch -> ([2, MAX_DET, H, W] planes on the host, the guard bands).  proto: NHWC [2, mh, mw, nm] host
    tensor (its dtype is the kernel's); coef [2, 7, nm], or levels (host [2, h, w, nm] maps) with keep [2, 7]."""
    from ydbl import _lib
    from ydbl.utils.ops import launch_process_mask, mask_window

    n, mh, mw, nm = proto.shape
    cs = nm + proto_pad
    pb = torch.full((n * mh * mw, cs), float("nan"), dtype=proto.dtype, device=DEV)
    pb[:, :nm] = proto.reshape(-1, nm).to(DEV)
    pv = _lib.View(pb.data_ptr(), n, mh, mw, nm, cs, _lib.dtype_code(proto.dtype))
    det = torch.full((n, MAX_DET, 6), float("nan"), device=DEV)
    det[:, :7, :4] = boxes.to(DEV)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    if form == "native":
        H, W = frame
        window, sx, sy, after = mask_window(mh, mw, frame), 1.0, 1.0, True
    else:
        H, W = frame if form == "up" else (mh, mw)
        window, after = (0, 0, mh, mw), False
        sx, sy = (torch.tensor(v, dtype=torch.float32).item() for v in (mw / frame[1], mh / frame[0]))
    band = H * W  # (odd sizes: planes and rows that are not 16-byte aligned)
    dt = torch.uint8 if u8 else torch.float32
    buf = torch.full((2 * band + n * MAX_DET * H * W,), FILL, dtype=dt, device=DEV)
    out = buf[band:band + n * MAX_DET * H * W]
    rows = torch.tensor([b * MAX_DET for b in range(n)], dtype=torch.int64, device=DEV)
    kw = {}
    hold = []
    if coef is not None:
        cf = torch.full((n, MAX_DET, nm), float("nan"), device=DEV)
        cf[:, :7] = coef.to(DEV)
        kw["coef"] = cf
    else:
        mcv = []
        for lv in levels:
            t = lv.to(DEV).contiguous()
            hold.append(t)
            mcv.append(_lib.View(t.data_ptr(), n, lv.shape[1], lv.shape[2], nm, nm, _lib.dtype_code(lv.dtype)))
        ki = torch.full((n, MAX_DET), -1, dtype=torch.int32, device=DEV)
        ki[:, :7] = keep.to(DEV)
        kw.update(mc=mcv, keep_idx=ki, nc=nc)
    launch_process_mask(pv, det, cnt, rows, out, (H, W), window=window, sx=sx, sy=sy, crop_after=after,
                        max_det=MAX_DET, **kw)
    torch.cuda.synchronize()
    host = buf.cpu()
    return host[band:band + n * MAX_DET * H * W].view(n, MAX_DET, H, W), (host[:band], host[-band:])


def check(form, got, bands, proto, coef, boxes, counts, frame):
    """The rule over a launch's planes; returns (near, pos) of the case."""
    v64, s64 = S.mask_reference(form, proto, coef, boxes, counts, frame)
    assert all((b == FILL).all() for b in bands)
    near_tot = pos_tot = 0
    for b, k in enumerate(counts):
        assert (got[b, k:] == FILL).all()  # planes past the count: untouched
        if k == 0:
            continue
        assert ((got[b, :k] == 0) | (got[b, :k] == 1)).all()
        wrong, near, pos = S.mask_check(got[b, :k], v64[b], s64[b])
        assert wrong == 0, (b, wrong)
        near_tot += near
        pos_tot += pos
    assert near_tot <= S.NEAR_ZERO_CAP * max(pos_tot, 1)
    return near_tot, pos_tot


def frame_of(form, mh, mw, shape):
    return shape if form == "native" else (4 * mh, 4 * mw)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("form,mh,mw,shape", S.MASK_FORMS)
def test_forms_direct_coefficients(form, mh, mw, shape, half):
    frame = frame_of(form, mh, mw, shape)
    boxes = S.mask_boxes(*frame)
    near_tot = pos_tot = 0
    for counts in S.MASK_COUNTS:
        proto, coef = S.mask_inputs(0, mh, mw, 32, half)
        got, bands = run(form, proto, boxes, counts, frame, coef=coef)
        near, pos = check(form, got, bands, proto, coef, boxes, counts, frame)
        near_tot, pos_tot = near_tot + near, pos_tot + pos
        again, _ = run(form, proto, boxes, counts, frame, coef=coef)
        assert torch.equal(got, again)  # bit-identical from run to run
        u8, bands8 = run(form, proto, boxes, counts, frame, coef=coef, u8=True)
        assert all((b == FILL).all() for b in bands8)
        assert torch.equal(u8.float(), got)  # both output types: the same masks (and the same untouched planes)
    print(f"mask {form} {mh}x{mw}->{shape} {'half' if half else 'fp32'}: near-zero {near_tot} / {pos_tot}")


@pytest.mark.parametrize("nc", [0, 3], ids=["anchor", "multi_label"])
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("form,mh,mw,shape", [S.MASK_FORMS[0], S.MASK_FORMS[3], S.MASK_FORMS[5]])
def test_coefficients_from_level_maps(form, mh, mw, shape, half, nc):
    """keep_idx -> anchor (-> anchor * nc + cls) -> the level map's row: the same masks as the gathered coefficients
    given directly, and the restatement's."""
    frame = frame_of(form, mh, mw, shape)
    boxes = S.mask_boxes(*frame)
    proto, _ = S.mask_inputs(1, mh, mw, 32, half)
    g = torch.Generator().manual_seed(5)
    levels = [torch.randn(2, h, w, 32, generator=g) for h, w in LEVELS]
    if half:
        levels = [lv.half() for lv in levels]
    A = sum(h * w for h, w in LEVELS)
    flat = torch.cat([lv.reshape(2, -1, 32) for lv in levels], 1).float()  # [2, A, nm], anchors level after level
    anchors = torch.stack([torch.randperm(A, generator=g)[:7] for _ in range(2)])
    anchors[0, 0], anchors[0, 1], anchors[1, 0] = 0, A - 1, LEVELS[0][0] * LEVELS[0][1]  # level edges
    coef = torch.stack([flat[b, anchors[b]] for b in range(2)])
    keep = anchors if nc == 0 else anchors * nc + torch.randint(0, nc, anchors.shape, generator=g)
    counts = (1, 7)
    got, bands = run(form, proto, boxes, counts, frame, levels=levels, keep=keep.int(), nc=nc)
    check(form, got, bands, proto, coef, boxes, counts, frame)
    direct, _ = run(form, proto, boxes, counts, frame, coef=coef)
    assert torch.equal(got, direct)


@pytest.mark.parametrize("form,mh,mw,shape", [S.MASK_FORMS[1], S.MASK_FORMS[2], S.MASK_FORMS[6]])
def test_nm8_and_a_padded_proto_stride(form, mh, mw, shape):
    frame = frame_of(form, mh, mw, shape)
    boxes = S.mask_boxes(*frame)
    for half in (False, True):
        proto, coef = S.mask_inputs(2, mh, mw, 8, half)
        got, bands = run(form, proto, boxes, (7, 1), frame, coef=coef, proto_pad=8)
        check(form, got, bands, proto, coef, boxes, (7, 1), frame)


def test_ops_entry_points_match_the_restatement():
    """ydbl.utils.ops.process_mask / process_mask_native (the reference signatures) on CUDA tensors."""
    from ydbl.utils import ops

    proto, coef = S.mask_inputs(3, 24, 40, 32, False)
    p = proto[0].permute(2, 0, 1).contiguous()
    for form, shape, fn in (("up", (96, 160), lambda b: ops.process_mask(p.to(DEV), coef[0].to(DEV), b.to(DEV),
                                                                         (96, 160), upsample=True)),
                            ("same", (96, 160), lambda b: ops.process_mask(p.to(DEV), coef[0].to(DEV), b.to(DEV),
                                                                           (96, 160))),
                            ("native", (101, 127), lambda b: ops.process_mask_native(p.half().to(DEV), coef[0].to(DEV),
                                                                                     b.to(DEV), (101, 127)))):
        boxes = S.mask_boxes(*shape)
        pr = proto.half() if form == "native" else proto
        got = fn(boxes).cpu()
        v64, s64 = S.mask_reference(form, pr, coef, boxes, (7, 0), shape)
        assert got.dtype == torch.float32 and got.shape == v64[0].shape
        wrong, near, pos = S.mask_check(got, v64[0], s64[0])
        assert wrong == 0 and near <= S.NEAR_ZERO_CAP * pos
    assert ops.process_mask(p.to(DEV), coef[0, :0].to(DEV), boxes[:0].to(DEV), (96, 160)).shape == (0, 24, 40)
    m = torch.randn(3, 24, 40)
    assert torch.equal(ops.crop_mask(m.to(DEV), boxes[:3].to(DEV) * 0.25).cpu(), S.crop_mask(m, boxes[:3] * 0.25))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.process_mask(p, coef[0], boxes, (96, 160))
