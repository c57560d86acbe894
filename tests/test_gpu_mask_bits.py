"""YDBL_MASK_BITS on the MI355X: ydbl_process_mask's bit planes equal np.packbits(bitorder="little") of the uint8
output of the same call -- over the forms, counts and both prototype types of tests/test_gpu_mask.py, which holds the
uint8 output to the restatement.  Widths 160 and 64 fill their words, 40, 127, 173 and 150 leave tail bits that must
be 0; planes past an image's count and the guard bands keep their fill."""

import numpy as np
import pytest
import torch

import seg_util as S
import segval_util as SV

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_DET = 9
FILL = 0x0707070707070707


def run(form, proto, boxes, counts, frame, coef, bits):
    """One launch with direct coefficients -> ([2, MAX_DET, H, W] uint8 or [2, MAX_DET, H, ceil(W / 64)] uint64 on the
    host, the two guard bands)."""
    from ydbl import _lib
    from ydbl.utils.ops import launch_process_mask, mask_window

    n, mh, mw, nm = proto.shape
    pb = proto.reshape(-1, nm).to(DEV).contiguous()
    pv = _lib.View(pb.data_ptr(), n, mh, mw, nm, nm, _lib.dtype_code(proto.dtype))
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
    per = H * ((W + 63) // 64) if bits else H * W
    band = per
    buf = torch.full((2 * band + n * MAX_DET * per,), FILL if bits else 7, dtype=torch.int64 if bits else torch.uint8,
                     device=DEV)
    out = buf[band:band + n * MAX_DET * per]
    rows = torch.tensor([b * MAX_DET for b in range(n)], dtype=torch.int64, device=DEV)
    cf = torch.full((n, MAX_DET, nm), float("nan"), device=DEV)
    cf[:, :7] = coef.to(DEV)
    launch_process_mask(pv, det, cnt, rows, out, (H, W), window=window, sx=sx, sy=sy, crop_after=after,
                        max_det=MAX_DET, coef=cf, out_dtype=_lib.MASK_BITS if bits else None)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    if bits:
        host = host.view(np.uint64)
    return host[band:band + n * MAX_DET * per].reshape(n, MAX_DET, H, -1), (host[:band], host[-band:])


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "half"])
@pytest.mark.parametrize("form,mh,mw,shape", S.MASK_FORMS)
def test_bits_equal_packed_u8(form, mh, mw, shape, half):
    frame = shape if form == "native" else (4 * mh, 4 * mw)
    boxes = S.mask_boxes(*frame)
    for counts in S.MASK_COUNTS:
        proto, coef = S.mask_inputs(0, mh, mw, 32, half)
        u8, b8 = run(form, proto, boxes, counts, frame, coef, bits=False)
        words, bw = run(form, proto, boxes, counts, frame, coef, bits=True)
        assert all((b == 7).all() for b in b8) and all((b == np.uint64(FILL)).all() for b in bw)
        W = u8.shape[-1]
        assert words.shape == (*u8.shape[:3], (W + 63) // 64)
        set_bits = 0
        for b, k in enumerate(counts):
            assert (words[b, k:] == np.uint64(FILL)).all() and (u8[b, k:] == 7).all()  # slots >= count: untouched
            if k:
                want = SV.pack_bits(u8[b, :k])
                assert np.array_equal(words[b, :k], want)
                if W % 64:  # the bits past out_w are 0
                    assert not (words[b, :k, :, -1] >> np.uint64(W % 64)).any()
                set_bits += int(u8[b, :k].sum())
        assert set_bits > 0
