"""ctypes binding of libydbl.so (the C ABI in include/ydbl.h).

There is no fallback: if the library is missing or cannot be loaded the
import raises, so a GPU run can never silently go through another path.
torch is imported first so that libydbl resolves ``libamdhip64.so.7`` to the
HIP runtime torch already loaded (one runtime, one set of streams).
"""

from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch  # noqa: F401  (must precede the dlopen below)

LIB_PATH = Path(os.environ.get("YDBL_LIB", Path(__file__).resolve().parent / "libydbl.so"))

F32, F16 = 0, 1
ACT_NONE, ACT_SILU, ACT_GELU, ACT_SIGMOID = 0, 1, 2, 3
RES_NONE, RES_ADD, RES_MUL = 0, 1, 2


class View(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("c", C.c_int32),
                ("cs", C.c_int32), ("dtype", C.c_int32)]


class ConvDesc(C.Structure):
    _fields_ = [("x", View), ("y", View), ("r", View), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("dil", C.c_int32),
                ("kpad", C.c_int32), ("act", C.c_int32), ("res_mode", C.c_int32),
                ("y2", View), ("r2", View), ("a2", C.c_float), ("b2", C.c_float),
                ("dq", C.c_void_p), ("qscale", C.c_float), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class ConvRouteInfo(C.Structure):
    """ydbl_conv_route_info: what ydbl_conv2d_nhwc would launch for a descriptor (include/ydbl.h ydbl_conv_route)."""
    _fields_ = [("family", C.c_int32), ("v", C.c_int32 * 4), ("pointwise", C.c_int32), ("ksplit", C.c_int32),
                ("epi", C.c_int32), ("grid", C.c_uint32 * 3), ("workspace_bytes", C.c_int64)]


CONV_VW, CONV_TILE, CONV_HALO, CONV_WSK, CONV_IGEMM = range(5)


class DwConvDesc(C.Structure):
    _fields_ = [("x", View), ("y", View), ("r", View), ("w", C.c_void_p), ("bias", C.c_void_p),
                ("kh", C.c_int32), ("kw", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32), ("dil", C.c_int32),
                ("act", C.c_int32), ("res_mode", C.c_int32)]


class DsConvDesc(C.Structure):
    _fields_ = [("x", View), ("y", View), ("r", View), ("dw_w", C.c_void_p), ("pw_w", C.c_void_p),
                ("bias", C.c_void_p), ("k", C.c_int32), ("stride", C.c_int32), ("pad", C.c_int32),
                ("dil", C.c_int32), ("kpad", C.c_int32), ("act", C.c_int32), ("res_mode", C.c_int32),
                ("dw_bias", C.c_void_p), ("dw_act", C.c_int32), ("tail_w", C.c_void_p), ("tail_b", C.c_void_p),
                ("tail_y", View), ("tail_n", C.c_int32),
                # the tail's NMS-candidate sink (include/ydbl.h): unset (cand_count NULL) unless a session fills it
                ("cand_box", C.c_void_p), ("cand_score", C.c_void_p), ("cand_cls", C.c_void_p),
                ("cand_idx", C.c_void_p), ("cand_count", C.c_void_p), ("cand_cap", C.c_int32),
                ("conf_thres", C.c_float), ("multi_label", C.c_int32), ("nclasses", C.c_int32),
                ("classes", C.c_void_p), ("level_stride", C.c_float), ("anchor0", C.c_int32), ("box", View),
                ("zero_counts", C.c_int32), ("y_unused", C.c_int32),
                # the sink's deferred mode (sparse box path): the candidates' 8 x 16 tiles flagged, no box read
                ("tile_mask", C.c_void_p), ("mask_tiles_x", C.c_int32), ("mask_tiles_img", C.c_int32),
                ("mask_zero", C.c_void_p), ("mask_zero_bytes", C.c_int32)]
    g2_w = g0_w = None  # not in the ABI: bench.py's roofline still asks every DSConv descriptor for these two


class HgDesc(C.Structure):
    _fields_ = [("x", View), ("xp", View), ("y", View), ("num_edges", C.c_int32), ("num_heads", C.c_int32),
                ("proto_base", C.c_void_p), ("ctx_w", C.c_void_p), ("ctx_b", C.c_void_p),
                ("edge_w", C.c_void_p), ("edge_b", C.c_void_p), ("node_w", C.c_void_p), ("node_b", C.c_void_p),
                ("workspace", C.c_void_p), ("pre_w", C.c_void_p), ("pre_b", C.c_void_p)]


class DecodeDesc(C.Structure):
    _fields_ = [("box", View * 3), ("cls", View * 3), ("nl", C.c_int32), ("nc", C.c_int32),
                ("stride", C.c_float * 3), ("conf_thres", C.c_float), ("multi_label", C.c_int32),
                ("classes", C.c_void_p), ("nclasses", C.c_int32), ("y_ref", C.c_void_p),
                ("cand_box", C.c_void_p), ("cand_score", C.c_void_p), ("cand_cls", C.c_void_p),
                ("cand_idx", C.c_void_p), ("cand_count", C.c_void_p), ("cap", C.c_int32)]


class DecodeAug(C.Structure):
    """ydbl_decode_aug: one test-time-augmentation pass's de-scale / de-flip / anchor window / merged position."""
    _fields_ = [("scale", C.c_float), ("flip_w", C.c_float), ("a_lo", C.c_int32), ("a_hi", C.c_int32),
                ("pos_base", C.c_int32), ("y_stride", C.c_int32), ("append", C.c_int32)]


class ScaleImgDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("n", C.c_int32), ("c", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("sh", C.c_int32), ("sw", C.c_int32), ("hp", C.c_int32), ("wp", C.c_int32), ("flip", C.c_int32),
                ("pad_value", C.c_float), ("y", C.c_void_p)]


class PredCandDesc(C.Structure):
    _fields_ = [("pred", C.c_void_p), ("n", C.c_int32), ("nc", C.c_int32), ("A", C.c_int32),
                ("conf_thres", C.c_float), ("multi_label", C.c_int32), ("classes", C.c_void_p),
                ("nclasses", C.c_int32), ("cand_box", C.c_void_p), ("cand_score", C.c_void_p),
                ("cand_cls", C.c_void_p), ("cand_idx", C.c_void_p), ("cand_count", C.c_void_p), ("cap", C.c_int32)]


class NmsDesc(C.Structure):
    _fields_ = [("cand_box", C.c_void_p), ("cand_score", C.c_void_p), ("cand_cls", C.c_void_p),
                ("cand_idx", C.c_void_p), ("cand_count", C.c_void_p), ("n", C.c_int32), ("cap", C.c_int32),
                ("iou_thres", C.c_double), ("max_det", C.c_int32), ("max_nms", C.c_int32), ("agnostic", C.c_int32),
                ("max_wh", C.c_float), ("clip_w", C.c_float), ("clip_h", C.c_float), ("out", C.c_void_p),
                ("out_count", C.c_void_p), ("workspace", C.c_void_p), ("out_stride", C.c_int64),
                ("count_stride", C.c_int64), ("per_image", C.c_int32), ("out_idx", C.c_void_p)]


class TopkDesc(C.Structure):
    """ydbl_topk_desc: the end2end head's selection (Detect.postprocess + the six-column NMS branch) over the decode's
    multi-label candidate lists; out / out_count as NmsDesc's."""
    _fields_ = [("cand_box", C.c_void_p), ("cand_score", C.c_void_p), ("cand_cls", C.c_void_p),
                ("cand_idx", C.c_void_p), ("cand_count", C.c_void_p), ("n", C.c_int32), ("cap", C.c_int32),
                ("k_head", C.c_int32), ("max_det", C.c_int32), ("classes", C.c_void_p), ("nclasses", C.c_int32),
                ("clip_w", C.c_float), ("clip_h", C.c_float), ("out", C.c_void_p), ("out_count", C.c_void_p),
                ("out_stride", C.c_int64), ("count_stride", C.c_int64), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64), ("per_image", C.c_int32)]


class InputBind(C.Structure):
    """ydbl_input_bind: device word holding the batch pointer, device fp32 batch maximum (LoadTensor's /255 rule)."""
    _fields_ = [("x", C.c_void_p), ("amax", C.c_void_p)]


class Stem2Desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("n", C.c_int32), ("cin", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("scale", C.c_float), ("c0", C.c_int32), ("params", C.c_void_p), ("y", View), ("bind", InputBind)]


class DySampleDesc(C.Structure):
    _fields_ = [("x", View), ("off", View), ("groups", C.c_int32), ("y", View), ("y2", View), ("r2", View),
                ("a2", C.c_float), ("b2", C.c_float)]


class DySample2Desc(C.Structure):
    _fields_ = [("x", View), ("off_w", C.c_void_p), ("off_b", C.c_void_p), ("groups", C.c_int32), ("y", View),
                ("y2", View), ("r2", View), ("a2", C.c_float), ("b2", C.c_float)]


class LskDesc(C.Structure):
    _fields_ = [("x", View), ("a1", View), ("a2", View), ("attn", View), ("y", View), ("w12", C.c_void_p),
                ("b12", C.c_void_p), ("sw", C.c_void_p), ("sb", C.c_void_p), ("w", C.c_void_p), ("b", C.c_void_p),
                ("agg", C.c_void_p)]


class BottleneckDesc(C.Structure):
    _fields_ = [("x", View), ("y", View), ("c", C.c_int32), ("add", C.c_int32), ("tile_h", C.c_int32),
                ("params", C.c_void_p), ("c_mid", C.c_int32), ("pw", C.c_int32),
                # sparse box launch (pw only): the tile mask and the candidate sink that decodes the boxes
                ("tile_mask", C.c_void_p), ("cand_box", C.c_void_p), ("cand_idx", C.c_void_p),
                ("cand_count", C.c_void_p), ("cand_cap", C.c_int32), ("level_stride", C.c_float),
                ("anchor0", C.c_int32), ("nc", C.c_int32), ("multi_label", C.c_int32)]


class LetterboxDesc(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_off", C.c_void_p), ("meta", C.c_void_p), ("n", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("pad_value", C.c_float), ("out", C.c_void_p)]


class MatchDesc(C.Structure):
    _fields_ = [("det", C.c_void_p), ("det_count", C.c_void_p), ("n", C.c_int32), ("max_det", C.c_int32),
                ("gt_box", C.c_void_p), ("gt_cls", C.c_void_p), ("gt_ofs", C.c_void_p), ("n_gt", C.c_int32),
                ("iouv", C.c_void_p), ("n_iou", C.c_int32), ("single_cls", C.c_int32), ("correct", C.c_void_p),
                ("workspace", C.c_void_p)]


class ConfusionDesc(C.Structure):
    _fields_ = [("det", C.c_void_p), ("det_count", C.c_void_p), ("n", C.c_int32), ("max_det", C.c_int32),
                ("gt_box", C.c_void_p), ("gt_cls", C.c_void_p), ("gt_ofs", C.c_void_p), ("n_gt", C.c_int32),
                ("nc", C.c_int32), ("conf", C.c_float), ("iou_thres", C.c_float), ("matrix", C.c_void_p),
                ("invalid", C.c_void_p), ("workspace", C.c_void_p)]


class CocoDesc(C.Structure):
    """ydbl_coco_desc: COCO-protocol matching over the det | count records and grouped labels (val(coco_eval=True));
    iou_thrs / area_rng are host fp64 arrays."""
    _fields_ = [("det", C.c_void_p), ("det_count", C.c_void_p), ("n", C.c_int32), ("max_det", C.c_int32),
                ("gt_box", C.c_void_p), ("gt_cls", C.c_void_p), ("gt_ofs", C.c_void_p), ("n_gt", C.c_int32),
                ("single_cls", C.c_int32), ("nc", C.c_int32), ("iou_thrs", C.c_void_p), ("n_iou", C.c_int32),
                ("area_rng", C.c_void_p), ("n_area", C.c_int32), ("max_dets", C.c_int32), ("dt_rank", C.c_void_p),
                ("dt_matched", C.c_void_p), ("dt_ignored", C.c_void_p), ("gt_ignore", C.c_void_p),
                ("invalid", C.c_void_p), ("workspace", C.c_void_p)]


class AreaAttnDesc(C.Structure):
    _fields_ = [("qkv", View), ("y", View), ("v", View), ("heads", C.c_int32), ("area", C.c_int32),
                ("scale", C.c_float)]


class PsaAttnDesc(C.Structure):
    """ydbl_psa_attn_desc: C2PSA's attention core, 128 channels per head (q 32 | k 32 | v 64)."""
    _fields_ = [("qkv", View), ("y", View), ("v", View), ("heads", C.c_int32), ("key_dim", C.c_int32),
                ("head_dim", C.c_int32), ("scale", C.c_float)]


class MaxPool5Desc(C.Structure):
    """ydbl_maxpool5_desc: SPPF's three cascaded MaxPool2d(5, 1, 2), one launch."""
    _fields_ = [("x", View), ("y1", View), ("y2", View), ("y3", View), ("k", C.c_int32)]


class AvgPoolDesc(C.Structure):
    """ydbl_avgpool_desc: global average pool of an NHWC view into rows of a [B, D] buffer (Model.embed)."""
    _fields_ = [("x", View), ("y", C.c_void_p), ("y_stride", C.c_int64), ("workspace", C.c_void_p),
                ("workspace_bytes", C.c_int64)]


class TrackDesc(C.Structure):
    """ydbl_track_desc: ByteTrack association over the det | count records of ydbl_nms (Model.track)."""
    _fields_ = [("det", C.c_void_p), ("det_count", C.c_void_p), ("n", C.c_int32), ("max_det", C.c_int32),
                ("det_stride", C.c_int64), ("count_stride", C.c_int64), ("hw", C.c_void_p),
                ("track_high_thresh", C.c_double), ("track_low_thresh", C.c_double),
                ("new_track_thresh", C.c_double), ("match_thresh", C.c_double), ("fuse_score", C.c_int32),
                ("track_buffer", C.c_int32), ("max_time_lost", C.c_int32), ("max_tracks", C.c_int32),
                ("trackers", C.c_int32), ("reset_each", C.c_int32), ("out", C.c_void_p), ("out_count", C.c_void_p),
                ("tracked", C.c_void_p), ("out_idx", C.c_void_p), ("state", C.c_void_p), ("state_bytes", C.c_int64)]


class LossDesc(C.Structure):
    """ydbl_loss_desc: the detection loss (TaskAlignedAssigner + CIoU / BCE / DFL) over the Detect levels in place."""
    _fields_ = [("box", View * 3), ("cls", View * 3), ("nl", C.c_int32), ("nc", C.c_int32), ("reg_max", C.c_int32),
                ("stride", C.c_float * 3), ("gt", C.c_void_p), ("max_labels", C.c_int32), ("topk", C.c_int32),
                ("gain_box", C.c_float), ("gain_cls", C.c_float), ("gain_dfl", C.c_float),
                ("loss", C.c_void_p), ("target_scores_sum", C.c_void_p), ("per_image", C.c_void_p),
                ("fg", C.c_void_p), ("target_gt_idx", C.c_void_p), ("target_score", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class LossGradDesc(C.Structure):
    """ydbl_loss_grad_desc: d(loss.sum() * batch_size) / d(level logits) given the assignment ydbl_detect_loss wrote."""
    _fields_ = [("box", View * 3), ("cls", View * 3), ("nl", C.c_int32), ("nc", C.c_int32), ("reg_max", C.c_int32),
                ("stride", C.c_float * 3), ("gt", C.c_void_p), ("max_labels", C.c_int32),
                ("gain_box", C.c_float), ("gain_cls", C.c_float), ("gain_dfl", C.c_float),
                ("fg", C.c_void_p), ("target_gt_idx", C.c_void_p), ("target_score", C.c_void_p),
                ("target_scores_sum", C.c_void_p), ("grad_scale", C.c_void_p), ("batch_scale", C.c_float),
                ("gbox", View * 3), ("gcls", View * 3)]


class DeconvDesc(C.Structure):
    """ydbl_deconv_desc: ConvTranspose2d(cin, cout, 2, 2) on NHWC views (Proto.upsample), packed weights."""
    _fields_ = [("x", View), ("y", View), ("w", C.c_void_p), ("bias", C.c_void_p), ("act", C.c_int32)]


MASK_F32, MASK_U8, MASK_BITS = 0, 1, 2


class MaskDesc(C.Structure):
    """ydbl_mask_desc: process_mask / process_mask_native for a batch, one launch."""
    _fields_ = [("proto", View), ("mc", View * 3), ("nl", C.c_int32), ("nc", C.c_int32), ("keep_idx", C.c_void_p),
                ("det", C.c_void_p), ("det_stride", C.c_int64), ("det_row", C.c_int32), ("max_det", C.c_int32),
                ("count", C.c_void_p), ("coef", C.c_void_p), ("row_offset", C.c_void_p), ("out", C.c_void_p),
                ("out_h", C.c_int32), ("out_w", C.c_int32), ("out_dtype", C.c_int32),
                ("top", C.c_int32), ("left", C.c_int32), ("bottom", C.c_int32), ("right", C.c_int32),
                ("sx", C.c_float), ("sy", C.c_float), ("crop_after", C.c_int32), ("slots", C.c_int32)]


class GtBitsDesc(C.Structure):
    """ydbl_gt_bits_desc: a batch's ground-truth masks (index map or planes) -> bit planes and areas."""
    _fields_ = [("src", C.c_void_p), ("n", C.c_int32), ("gh", C.c_int32), ("gw", C.c_int32), ("overlap", C.c_int32),
                ("gt_ofs", C.c_void_p), ("n_gt", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("bits", C.c_void_p), ("area", C.c_void_p)]


class MaskIouDesc(C.Structure):
    """ydbl_mask_iou_desc: mask IoU of every label against the detection slots of its image, on bit planes."""
    _fields_ = [("det_bits", C.c_void_p), ("row_offset", C.c_void_p), ("count", C.c_void_p), ("n", C.c_int32),
                ("max_det", C.c_int32), ("gt_bits", C.c_void_p), ("gt_ofs", C.c_void_p), ("area_gt", C.c_void_p),
                ("n_gt", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32), ("iou", C.c_void_p),
                ("inter", C.c_void_p), ("area_det", C.c_void_p)]


class MatchIouDesc(C.Structure):
    """ydbl_match_iou_desc: ydbl_match_predictions' rule on a given IoU matrix [n_gt][max_det]."""
    _fields_ = [("det", C.c_void_p), ("det_count", C.c_void_p), ("n", C.c_int32), ("max_det", C.c_int32),
                ("iou", C.c_void_p), ("gt_cls", C.c_void_p), ("gt_ofs", C.c_void_p), ("n_gt", C.c_int32),
                ("iouv", C.c_void_p), ("n_iou", C.c_int32), ("single_cls", C.c_int32), ("correct", C.c_void_p),
                ("workspace", C.c_void_p)]


class PoseKptDesc(C.Structure):
    """ydbl_pose_kpt_desc: the kept detections' keypoints, decoded in fp32 from the level maps keep_idx names."""
    _fields_ = [("kpt", View * 3), ("nl", C.c_int32), ("nc", C.c_int32), ("stride", C.c_float * 3),
                ("keep_idx", C.c_void_p), ("count", C.c_void_p), ("n", C.c_int32), ("max_det", C.c_int32),
                ("K", C.c_int32), ("ndim", C.c_int32), ("out", C.c_void_p)]


class KptOksDesc(C.Structure):
    """ydbl_kpt_oks_desc: OKS of every label against the detection slots of its image -> [n_gt][max_det]."""
    _fields_ = [("pred_kpts", C.c_void_p), ("count", C.c_void_p), ("n", C.c_int32), ("max_det", C.c_int32),
                ("K", C.c_int32), ("ndim", C.c_int32), ("gt_kpts", C.c_void_p), ("gt_box", C.c_void_p),
                ("gt_ofs", C.c_void_p), ("n_gt", C.c_int32), ("sigma", C.c_void_p), ("oks", C.c_void_p)]


# name -> (argtypes, restype); every entry must exist in include/ydbl.h
_P = C.c_void_p
_VP = C.POINTER(View)
SIGNATURES = {
    "ydbl_conv2d_nhwc": ([C.POINTER(ConvDesc), _P], C.c_int),
    "ydbl_dwconv2d_nhwc": ([C.POINTER(DwConvDesc), _P], C.c_int),
    "ydbl_dwconv2d_pair_nhwc": ([C.POINTER(DwConvDesc), C.POINTER(DwConvDesc), _P], C.c_int),
    "ydbl_dwconv2d_pair_route": ([C.POINTER(DwConvDesc), C.POINTER(DwConvDesc)], C.c_int),
    "ydbl_dsconv_nhwc": ([C.POINTER(DsConvDesc), _P], C.c_int),
    "ydbl_batch_max_work_ints": ([], C.c_int32),
    "ydbl_batch_max_work_init": ([_P], None),
    "ydbl_batch_max": ([_P, C.c_int64, _P, _P, _P, _P], C.c_int),
    "ydbl_batch_max_bound": ([_P, C.c_int64, _P, _P, _P, _P], C.c_int),
    "ydbl_input_nchw_to_nhwc": ([_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _VP,
                                 C.POINTER(InputBind), _P], C.c_int),
    "ydbl_conv_stem": ([_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P, _P, C.c_int32, C.c_int32,
                        C.c_int32, _VP, C.POINTER(InputBind), _P], C.c_int),
    "ydbl_gate_add": ([_VP, _VP, C.c_float, _VP, _P], C.c_int),
    "ydbl_channel_gate_add": ([_VP, _VP, _P, _VP, _P], C.c_int),
    "ydbl_area_attn": ([C.POINTER(AreaAttnDesc), _P], C.c_int),
    "ydbl_psa_attn": ([C.POINTER(PsaAttnDesc), _P], C.c_int),
    "ydbl_maxpool5_cascade": ([C.POINTER(MaxPool5Desc), _P], C.c_int),
    "ydbl_pool_up_concat": ([_VP, _VP, _VP, _VP, _P], C.c_int),
    "ydbl_dysample": ([_VP, _VP, C.c_int32, _VP, _P], C.c_int),
    "ydbl_dysample_ex": ([C.POINTER(DySampleDesc), _P], C.c_int),
    "ydbl_lsk_gate": ([_VP, _P, _P, _VP, _P, _P], C.c_int),
    "ydbl_lsk_gate_workspace": ([C.c_int32, C.c_int32, C.c_int32], C.c_int64),
    "ydbl_lsk_attn": ([C.POINTER(LskDesc), _P], C.c_int),
    "ydbl_lsk_out": ([C.POINTER(LskDesc), _P], C.c_int),
    "ydbl_hg_workspace": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32], C.c_int64),
    "ydbl_hg_context": ([C.POINTER(HgDesc), _P], C.c_int),
    "ydbl_hg_propagate": ([C.POINTER(HgDesc), _P], C.c_int),
    "ydbl_hg_fused_workspace": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32], C.c_int64),
    "ydbl_hg_fused": ([C.POINTER(HgDesc), _P], C.c_int),
    "ydbl_hg_fused_pair": ([C.POINTER(HgDesc), C.POINTER(HgDesc), _P], C.c_int),
    "ydbl_dysample2": ([C.POINTER(DySample2Desc), _P], C.c_int),
    "ydbl_detect_decode": ([C.POINTER(DecodeDesc), _P], C.c_int),
    "ydbl_detect_decode_aug": ([C.POINTER(DecodeDesc), C.POINTER(DecodeAug), _P], C.c_int),
    "ydbl_detect_decode_e2e": ([C.POINTER(DecodeDesc), _P], C.c_int),
    "ydbl_detect_topk_workspace": ([C.c_int32, C.c_int32], C.c_int64),
    "ydbl_detect_topk": ([C.POINTER(TopkDesc), _P], C.c_int),
    "ydbl_scale_img": ([C.POINTER(ScaleImgDesc), _P], C.c_int),
    "ydbl_pred_candidates": ([C.POINTER(PredCandDesc), _P], C.c_int),
    "ydbl_nms_workspace": ([C.c_int32, C.c_int32, C.c_int32], C.c_int64),
    "ydbl_conv_workspace": ([C.POINTER(ConvDesc)], C.c_int64),
    "ydbl_conv_route": ([C.POINTER(ConvDesc), C.POINTER(ConvRouteInfo)], C.c_int),
    "ydbl_nms": ([C.POINTER(NmsDesc), _P], C.c_int),
    "ydbl_conv_stem2_params_size": ([C.c_int32], C.c_int64),
    "ydbl_conv_stem2_pack": ([_P, _P, _P, _P, C.c_int32, _P], C.c_int),
    "ydbl_conv_stem2": ([C.POINTER(Stem2Desc), _P], C.c_int),
    "ydbl_bottleneck_params_size": ([C.c_int32], C.c_int64),
    "ydbl_bottleneck_pack": ([_P, _P, _P, _P, C.c_int32, _P], C.c_int),
    "ydbl_bottleneck_nhwc": ([C.POINTER(BottleneckDesc), _P], C.c_int),
    "ydbl_conv3x3_pair_params_size": ([C.c_int32, C.c_int32], C.c_int64),
    "ydbl_conv3x3_pair_pack": ([_P, _P, _P, _P, C.c_int32, C.c_int32, _P], C.c_int),
    "ydbl_detect_box_params_size": ([C.c_int32, C.c_int32], C.c_int64),
    "ydbl_detect_box_pack": ([_P, _P, _P, _P, _P, _P, C.c_int32, C.c_int32, _P], C.c_int),
    "ydbl_letterbox": ([C.POINTER(LetterboxDesc), _P], C.c_int),
    "ydbl_match_workspace": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32], C.c_int64),
    "ydbl_match_predictions": ([C.POINTER(MatchDesc), _P], C.c_int),
    "ydbl_confusion_workspace": ([C.c_int32, C.c_int32, C.c_int32], C.c_int64),
    "ydbl_confusion_matrix": ([C.POINTER(ConfusionDesc), _P], C.c_int),
    "ydbl_coco_workspace": ([C.c_int32, C.c_int32, C.c_int32, C.c_int32], C.c_int64),
    "ydbl_coco_match": ([C.POINTER(CocoDesc), _P], C.c_int),
    "ydbl_global_avgpool_workspace": ([C.POINTER(AvgPoolDesc)], C.c_int64),
    "ydbl_global_avgpool": ([C.POINTER(AvgPoolDesc), _P], C.c_int),
    "ydbl_bytetrack_state_bytes": ([C.c_int32, C.c_int32], C.c_int64),
    "ydbl_bytetrack_update": ([C.POINTER(TrackDesc), _P], C.c_int),
    "ydbl_detect_loss_workspace": ([C.c_int32, C.c_int32, C.c_int32], C.c_int64),
    "ydbl_detect_loss": ([C.POINTER(LossDesc), _P], C.c_int),
    "ydbl_detect_loss_grad": ([C.POINTER(LossGradDesc), _P], C.c_int),
    "ydbl_deconv2x2_nhwc": ([C.POINTER(DeconvDesc), _P], C.c_int),
    "ydbl_process_mask": ([C.POINTER(MaskDesc), _P], C.c_int),
    "ydbl_gt_mask_bits": ([C.POINTER(GtBitsDesc), _P], C.c_int),
    "ydbl_mask_iou": ([C.POINTER(MaskIouDesc), _P], C.c_int),
    "ydbl_match_iou": ([C.POINTER(MatchIouDesc), _P], C.c_int),
    "ydbl_pose_keypoints": ([C.POINTER(PoseKptDesc), _P], C.c_int),
    "ydbl_kpt_oks": ([C.POINTER(KptOksDesc), _P], C.c_int),
    "ydbl_last_error": ([], C.c_char_p),
    "ydbl_version": ([], C.c_char_p),
}


def _load():
    if not LIB_PATH.exists():
        raise ImportError(
            f"libydbl.so not found at {LIB_PATH}; build it with `python -c \"import __graft_entry__ as g; g.build()\"` "
            "(the HIP path has no fallback)"
        )
    lib = C.CDLL(str(LIB_PATH))
    for name, (args, res) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    return lib


lib = _load()


class YdblError(RuntimeError):
    pass


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib.ydbl_last_error().decode(errors="replace")
        raise YdblError(f"{what or 'ydbl'} failed (code {rc}): {msg}")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float16:
        return F16
    if dt == torch.float32:
        return F32
    raise TypeError(f"unsupported activation dtype {dt}")


def version() -> str:
    return lib.ydbl_version().decode()


def batch_max_work(device) -> "torch.Tensor":
    """A ready work buffer for ydbl_batch_max on `device` (include/ydbl.h)."""
    import torch

    host = torch.empty(int(lib.ydbl_batch_max_work_ints()), dtype=torch.int32)
    lib.ydbl_batch_max_work_init(host.data_ptr())
    return host.to(device)
