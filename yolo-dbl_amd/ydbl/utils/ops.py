"""Box utilities and HIP-backed NMS with the reference signature (U/utils/ops.py)."""

from __future__ import annotations

import math

import torch

from .. import _lib
from .._lib import NmsDesc, PredCandDesc
from ..tail import CandidateLists, nms_workspace


def make_divisible(x, divisor):
    """U/utils/ops.py:130-143."""
    if isinstance(divisor, torch.Tensor):
        divisor = int(divisor.max())
    return math.ceil(x / divisor) * divisor


def xywh2xyxy(x):
    """U/utils/ops.py:416-433."""
    assert x.shape[-1] == 4, f"input shape last dimension expected 4 but input shape is {x.shape}"
    y = torch.empty_like(x, dtype=torch.float32)
    xy = x[..., :2]
    wh = x[..., 2:] / 2
    y[..., :2] = xy - wh
    y[..., 2:] = xy + wh
    return y


def clip_boxes(boxes, shape):
    """U/utils/ops.py:319-338."""
    boxes[..., 0] = boxes[..., 0].clamp(0, shape[1])
    boxes[..., 1] = boxes[..., 1].clamp(0, shape[0])
    boxes[..., 2] = boxes[..., 2].clamp(0, shape[1])
    boxes[..., 3] = boxes[..., 3].clamp(0, shape[0])
    return boxes


def scale_boxes(img1_shape, boxes, img0_shape, ratio_pad=None, padding=True, xywh=False):
    """U/utils/ops.py:92-127."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1),
               round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    if padding:
        boxes[..., 0] -= pad[0]
        boxes[..., 1] -= pad[1]
        if not xywh:
            boxes[..., 2] -= pad[0]
            boxes[..., 3] -= pad[1]
    boxes[..., :4] /= gain
    return clip_boxes(boxes, img0_shape)


def clip_coords(coords, shape):
    """U/utils/ops.py:341-358: x to [0, shape[1]], y to [0, shape[0]], in place (tensor or ndarray)."""
    if isinstance(coords, torch.Tensor):
        coords[..., 0] = coords[..., 0].clamp(0, shape[1])
        coords[..., 1] = coords[..., 1].clamp(0, shape[0])
    else:
        coords[..., 0] = coords[..., 0].clip(0, shape[1])
        coords[..., 1] = coords[..., 1].clip(0, shape[0])
    return coords


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None, normalize=False, padding=True):
    """U/utils/ops.py:740-772: point coordinates (x, y in the first two columns) from the letterboxed img1_shape to
    img0_shape, in place.  Unlike scale_boxes the pad is NOT rounded."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    if padding:
        coords[..., 0] -= pad[0]
        coords[..., 1] -= pad[1]
    coords[..., 0] /= gain
    coords[..., 1] /= gain
    coords = clip_coords(coords, img0_shape)
    if normalize:
        coords[..., 0] /= img0_shape[1]
        coords[..., 1] /= img0_shape[0]
    return coords


def kpt_oks(pred_kpts, count, gt_kpts, gt_box, gt_ofs, sigma, stream=None):
    """One ydbl_kpt_oks launch (include/ydbl.h): pred_kpts fp32 [B, max_det, K, ndim] and count int32 [B] (a
    session's kpts / count, or copies brought to the labels' space) against gt_kpts fp32 [n_gt, K, 3] with the label
    boxes gt_box fp32 [n_gt, 4] xyxy, grouped by gt_ofs int32 [B + 1]; sigma fp32 [K]; all on the device.
    -> oks fp32 [n_gt, max_det] (row g: label g against the slots of its own image; columns >= count are 0)."""
    dev = pred_kpts.device
    n, max_det, K, ndim = pred_kpts.shape
    n_gt = gt_kpts.shape[0]
    for t, dt in ((pred_kpts, torch.float32), (gt_kpts, torch.float32), (gt_box, torch.float32),
                  (sigma, torch.float32), (count, torch.int32), (gt_ofs, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError("kpt_oks: contiguous fp32 / int32 tensors on one device expected")
    if tuple(gt_kpts.shape[1:]) != (K, 3) or tuple(gt_box.shape) != (n_gt, 4) or sigma.numel() != K \
            or count.numel() != n or gt_ofs.numel() != n + 1:
        raise ValueError("kpt_oks: gt_kpts [n_gt, K, 3], gt_box [n_gt, 4], sigma [K], count [B], gt_ofs [B + 1] expected")
    oks = torch.empty((max(n_gt, 1), max_det), dtype=torch.float32, device=dev)
    d = _lib.KptOksDesc(pred_kpts.data_ptr(), count.data_ptr(), n, max_det, K, ndim,
                        gt_kpts.data_ptr() if n_gt else None, gt_box.data_ptr() if n_gt else None, gt_ofs.data_ptr(),
                        n_gt, sigma.data_ptr(), oks.data_ptr())
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib.ydbl_kpt_oks(d, stream), "ydbl_kpt_oks")
    return oks[:n_gt]


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False,
                        multi_label=False, labels=(), max_det=300, nc=0, max_time_img=0.05, max_nms=30000,
                        max_wh=7680, in_place=True, rotated=False):
    """U/utils/ops.py:167-316 on the GPU: ydbl_pred_candidates + ydbl_nms.

    prediction: CUDA tensor [B, 4+nc, A] (xywh pixels, class scores), or a (pred, feats) tuple.
    Returns a list of [n_i, 6] CUDA tensors (x1, y1, x2, y2, conf, cls).  The reference's NMS time
    limit (max_time_img) never truncates here; masks, apriori labels and rotated boxes are not on
    the DBL path and raise.  The prediction tensor is not modified (in_place has no effect).
    """
    assert 0 <= conf_thres <= 1, f"Invalid Confidence threshold {conf_thres}, valid values are between 0.0 and 1.0"
    assert 0 <= iou_thres <= 1, f"Invalid IoU {iou_thres}, valid values are between 0.0 and 1.0"
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    if rotated or (labels is not None and len(labels)):
        raise NotImplementedError("rotated / autolabel NMS is not on the YOLO-DBL path")
    if prediction.shape[-1] == 6:
        # an end2end model's output [B, N, 6] (U/utils/ops.py:224-228): rows already selected and ordered by the head's
        # top-k, so only the threshold, the cut and the class filter remain -- the reference's three lines, on whatever
        # device the rows are (the sessions do this step inside ydbl_detect_topk; nothing here is a hot path)
        output = [pred[pred[:, 4] > conf_thres][:max_det] for pred in prediction]
        if classes is not None:
            cls_t = torch.tensor(list(classes), device=prediction.device)
            output = [pred[(pred[:, 5:6] == cls_t).any(1)] for pred in output]
        return output
    if not prediction.is_cuda:
        raise RuntimeError("ydbl non_max_suppression runs on the GPU only (prediction must be a CUDA tensor)")
    bs = prediction.shape[0]
    nc = nc or (prediction.shape[1] - 4)
    if prediction.shape[1] != 4 + nc:
        raise NotImplementedError("mask channels are not on the YOLO-DBL path")
    A = prediction.shape[2]
    multi_label = bool(multi_label) and nc > 1
    pred = prediction.detach().float().contiguous()
    dev = pred.device
    cands = CandidateLists(bs, CandidateLists.capacity(A, nc, multi_label), dev)
    cls_t = torch.tensor(list(classes), dtype=torch.int32, device=dev) if classes is not None else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    pd = PredCandDesc(pred.data_ptr(), bs, nc, A, float(conf_thres), int(multi_label),
                      cls_t.data_ptr() if cls_t is not None else None, len(cls_t) if cls_t is not None else 0,
                      **cands.fields())
    _lib.check(_lib.lib.ydbl_pred_candidates(pd, stream), "ydbl_pred_candidates")
    out = torch.zeros((bs, max_det, 6), dtype=torch.float32, device=dev)
    cnt = torch.zeros((bs,), dtype=torch.int32, device=dev)
    ws = nms_workspace(bs, cands.cap, max_nms, dev)
    nd = NmsDesc(n=bs, iou_thres=float(iou_thres), max_det=int(max_det), max_nms=int(max_nms),
                 agnostic=int(bool(agnostic)), max_wh=float(max_wh), out=out.data_ptr(), out_count=cnt.data_ptr(),
                 workspace=ws.data_ptr(), **cands.fields())
    _lib.check(_lib.lib.ydbl_nms(nd, stream), "ydbl_nms")
    counts = cnt.tolist()
    return [out[i, : counts[i]] for i in range(bs)]


# ----------------------------------------------------------------------------- instance masks (U/utils/ops.py:644-737)
MASK_MAX_DET = 4096  # ydbl_process_mask: detection slots per image and launch


def mask_dtype_code(dtype) -> int:
    """ydbl_mask_desc.out_dtype of a torch dtype: float32 (the reference's masks) or uint8."""
    if dtype in (None, torch.float32):
        return _lib.MASK_F32
    if dtype == torch.uint8:
        return _lib.MASK_U8
    raise ValueError(f"mask_dtype {dtype}: torch.float32 or torch.uint8 expected")


def mask_window(mh: int, mw: int, shape, padding: bool = True) -> tuple:
    """scale_masks' crop of an (mh, mw) grid for a target `shape` (U/utils/ops.py:726-734): (top, left, bottom,
    right), the letterbox padding on the proto grid cut away.  Python float arithmetic, as the reference's."""
    gain = min(mh / shape[0], mw / shape[1])
    pad = [mw - shape[1] * gain, mh - shape[0] * gain]
    if padding:
        pad[0] /= 2
        pad[1] /= 2
    top, left = (int(pad[1]), int(pad[0])) if padding else (0, 0)
    bottom, right = int(mh - pad[1]), int(mw - pad[0])
    return top, left, bottom, right


def launch_process_mask(proto, det, count, row_offset, out, out_hw, *, window, sx, sy, crop_after, max_det,
                        det_stride=0, det_row=0, coef=None, keep_idx=None, mc=(), nc=0, slots=0, stream=None,
                        out_dtype=None):
    """One ydbl_process_mask launch (include/ydbl.h).  proto: a _lib.View [n, mh, mw, nm]; det / count / row_offset /
    out / coef / keep_idx: device tensors or raw pointers; mc: the level Views when keep_idx names the anchors.
    out_dtype: a _lib.MASK_* code; None takes it from `out` (float32 or uint8).  _lib.MASK_BITS writes bit planes of
    out_h * ceil(out_w / 64) 64-bit words, for which `out` is an int64 tensor."""
    ptr = lambda t: t.data_ptr() if isinstance(t, torch.Tensor) else t  # noqa: E731
    d = _lib.MaskDesc()
    d.proto = proto
    for i, v in enumerate(mc):
        d.mc[i] = v
    d.nl, d.nc, d.keep_idx = len(mc), int(nc), ptr(keep_idx)
    d.det, d.det_stride, d.det_row, d.max_det = ptr(det), int(det_stride), int(det_row), int(max_det)
    d.count, d.coef, d.row_offset, d.out = ptr(count), ptr(coef), ptr(row_offset), ptr(out)
    d.out_h, d.out_w = int(out_hw[0]), int(out_hw[1])
    if out_dtype is not None:
        d.out_dtype = int(out_dtype)
    else:
        d.out_dtype = mask_dtype_code(out.dtype) if isinstance(out, torch.Tensor) else _lib.MASK_F32
    d.top, d.left, d.bottom, d.right = (int(v) for v in window)
    d.sx, d.sy, d.crop_after, d.slots = float(sx), float(sy), int(bool(crop_after)), int(slots)
    if stream is None:
        stream = torch.cuda.current_stream(out.device).cuda_stream
    _lib.check(_lib.lib.ydbl_process_mask(d, stream), "ydbl_process_mask")


def gt_mask_bits(src, gt_ofs, n_gt: int, out_hw, overlap: bool = True, stream=None):
    """One ydbl_gt_mask_bits launch (include/ydbl.h): a batch's ground-truth masks -> bit planes at out_hw.
    src: uint8 device tensor, the index map [B, gh, gw] (overlap: value l + 1 marks image b's l-th label) or planes
    [n_gt, gh, gw] in grouped label order; gt_ofs: int32 [B + 1] on the device (group_labels).  -> (words int64
    [n_gt, H, ceil(W / 64)], area int32 [n_gt]).  Equal to the reference's F.interpolate(...) > 0.5 wherever its
    value is not within rounding of 0.5 -- always at the exact ratio 4 of mask_ratio."""
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3):
        raise ValueError("gt_mask_bits: src must be a uint8 CUDA tensor [B | n_gt, gh, gw]")
    src = src.contiguous()
    dev = src.device
    H, W = int(out_hw[0]), int(out_hw[1])
    n = gt_ofs.numel() - 1
    if src.shape[0] != (n if overlap else n_gt):
        raise ValueError(f"gt_mask_bits: {src.shape[0]} maps for {n if overlap else n_gt} "
                         f"{'images' if overlap else 'labels'}")
    bits = torch.empty((n_gt, H, (W + 63) // 64), dtype=torch.int64, device=dev)
    area = torch.empty(n_gt, dtype=torch.int32, device=dev)
    if n_gt == 0:
        return bits, area
    d = _lib.GtBitsDesc(src.data_ptr(), n, src.shape[1], src.shape[2], int(bool(overlap)), gt_ofs.data_ptr(), n_gt,
                        H, W, bits.data_ptr(), area.data_ptr())
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib.ydbl_gt_mask_bits(d, stream), "ydbl_gt_mask_bits")
    return bits, area


def mask_iou_bits(det_bits, row_offset, count, max_det: int, gt_bits, gt_ofs, area_gt, out_hw, *, counts=False,
                  stream=None):
    """One ydbl_mask_iou launch (include/ydbl.h): detection bit planes (session.masks_bits) against ground-truth bit
    planes (gt_mask_bits).  row_offset int64 [B], count int32 [B], gt_ofs int32 [B + 1] on the device.
    -> iou fp32 [n_gt, max_det] (row g: label g against the slots of its own image; columns >= count are 0), and with
    counts=True also (inter int32 [n_gt, max_det], area_det int32 [B, max_det])."""
    dev = det_bits.device
    n, n_gt = count.numel(), area_gt.numel()
    # (a batch without labels still launches, for area_det: its empty outputs are cut from one-row buffers)
    iou = torch.empty((max(n_gt, 1), max_det), dtype=torch.float32, device=dev)
    inter = torch.empty((max(n_gt, 1), max_det), dtype=torch.int32, device=dev) if counts else None
    area_det = torch.empty((n, max_det), dtype=torch.int32, device=dev) if counts else None
    d = _lib.MaskIouDesc(det_bits.data_ptr(), row_offset.data_ptr(), count.data_ptr(), n, int(max_det),
                         gt_bits.data_ptr() if n_gt else None, gt_ofs.data_ptr(), area_gt.data_ptr() if n_gt else None,
                         n_gt, int(out_hw[0]), int(out_hw[1]), iou.data_ptr(),
                         inter.data_ptr() if counts else None, area_det.data_ptr() if counts else None)
    if stream is None:
        stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(_lib.lib.ydbl_mask_iou(d, stream), "ydbl_mask_iou")
    return (iou[:n_gt], inter[:n_gt], area_det) if counts else iou[:n_gt]


def pack_mask_bits(masks: torch.Tensor) -> torch.Tensor:
    """0 / 1 masks [N, ..., W] -> int64 words [N, ..., ceil(W / 64)] in the YDBL_MASK_BITS layout (bit j of word q =
    element 64 q + j), with torch ops on the masks' device."""
    w = masks.shape[-1]
    m = (masks != 0).to(torch.int64)
    pad = (-w) % 64
    if pad:
        m = torch.nn.functional.pad(m, (0, pad))
    m = m.view(*m.shape[:-1], -1, 64)
    shifts = torch.arange(64, dtype=torch.int64, device=m.device)
    return (m << shifts).sum(-1)  # distinct bits: the sum is the OR (bit 63 wraps to the sign bit, as intended)


def _masks_direct(protos, masks_in, bboxes, out_hw, window, sx, sy, crop_after):
    """process_mask / process_mask_native of one image on the GPU: protos [c, mh, mw], masks_in [n, c], bboxes
    [n, 4] -> fp32 0 / 1 masks [n, H, W].  More than MASK_MAX_DET rows go in several launches."""
    if not (isinstance(protos, torch.Tensor) and protos.is_cuda):
        raise RuntimeError("ydbl mask ops run on the GPU only (protos must be a CUDA tensor)")
    if protos.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"protos dtype {protos.dtype}: float32 or float16 expected")
    c, mh, mw = protos.shape
    n = masks_in.shape[0]
    dev = protos.device
    out = torch.empty((n, int(out_hw[0]), int(out_hw[1])), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    p = protos.permute(1, 2, 0).contiguous()  # NHWC, one image
    pv = _lib.View(p.data_ptr(), 1, mh, mw, c, c, _lib.dtype_code(p.dtype))
    coef = masks_in.detach().to(dev, torch.float32).contiguous()
    box = bboxes.detach().to(dev, torch.float32)[:, :4].contiguous()
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    for a in range(0, n, MASK_MAX_DET):
        k = min(MASK_MAX_DET, n - a)
        cnt = torch.full((1,), k, dtype=torch.int32, device=dev)
        launch_process_mask(pv, box[a:a + k], cnt, zero, out[a:a + k], out_hw, window=window, sx=sx, sy=sy,
                            crop_after=crop_after, max_det=k, det_row=4, coef=coef[a:a + k])
    return out


def crop_mask(masks, boxes):
    """U/utils/ops.py:644-658: masks [n, h, w] times the box indicator (r >= x1, r < x2, c >= y1, c < y2 on float
    indices).  Elementwise torch on the tensors' device; the mask path proper fuses it (ydbl_process_mask)."""
    _, h, w = masks.shape
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    r = torch.arange(w, device=masks.device, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, device=masks.device, dtype=x1.dtype)[None, :, None]
    return masks * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


def process_mask(protos, masks_in, bboxes, shape, upsample=False):
    """U/utils/ops.py:661-693 as one ydbl_process_mask launch: protos [c, mh, mw] (fp16 / fp32, CUDA), masks_in
    [n, c], bboxes [n, 4] in `shape` = (ih, iw) pixels -> fp32 0 / 1 masks [n, ih, iw] (upsample) or [n, mh, mw]."""
    c, mh, mw = protos.shape
    ih, iw = shape
    sx = torch.tensor(mw / iw, dtype=torch.float32).item()  # the ratio as torch multiplies it into an fp32 tensor
    sy = torch.tensor(mh / ih, dtype=torch.float32).item()
    out_hw = (ih, iw) if upsample else (mh, mw)
    return _masks_direct(protos, masks_in, bboxes, out_hw, (0, 0, mh, mw), sx, sy, False)


def process_mask_native(protos, masks_in, bboxes, shape):
    """U/utils/ops.py:696-713: the proto-grid masks resampled to `shape` through scale_masks' window, cropped to the
    boxes (in `shape` pixels) afterwards -> fp32 0 / 1 masks [n, shape[0], shape[1]]."""
    c, mh, mw = protos.shape
    return _masks_direct(protos, masks_in, bboxes, shape, mask_window(mh, mw, shape), 1.0, 1.0, True)


def scale_masks(masks, shape, padding=True):
    """U/utils/ops.py:716-737: masks [N, C, H, W] cropped to mask_window and resampled bilinearly to `shape`, values
    kept (no threshold) -- torch's own interpolate on the tensors' device; ydbl_process_mask does the same resampling
    fused with the coefficient product and the threshold."""
    mh, mw = masks.shape[2:]
    top, left, bottom, right = mask_window(mh, mw, shape, padding)
    masks = masks[..., top:bottom, left:right]
    return torch.nn.functional.interpolate(masks, shape, mode="bilinear", align_corners=False)
