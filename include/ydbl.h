/*
 * ydbl.h — C ABI of libydbl.so, the MI355X (gfx950) kernels behind the
 * YOLO-DBL inference hot path (backbone/neck conv stack, Detect decode,
 * class-wise NMS).
 *
 * Boundary rules:
 *   - every entry point is stateless and reentrant, takes caller-owned DEVICE
 *     pointers plus an explicit hipStream_t (passed as void*), and only
 *     enqueues work on that stream (graph-capturable: no malloc, no sync);
 *   - the return value is 0 on success, otherwise a YDBL_E* code, and
 *     ydbl_last_error() returns a thread-local message (the Python layer
 *     raises RuntimeError with it, mirroring the reference's exceptions /
 *     asserts, e.g. U/utils/ops.py:217-218, U/data/loaders.py:554-560);
 *   - activations are NHWC.  A "view" is (pointer, N, H, W, C, channel
 *     stride cs): element (n,y,x,c) lives at ptr[((n*H+y)*W+x)*cs + c].
 *     Writing into a channel slice of a wider buffer (cs > C) is how Concat,
 *     chunk() and C2f/C3 concatenations are done without copies.
 *
 * Reference interfaces replaced (paths relative to
 * /root/reference/models/YOLO/ultralytics):
 *   ydbl_conv2d_nhwc       <- nn/modules/conv.py:39-63 Conv.forward_fuse (conv+bias+SiLU after
 *                             nn/tasks.py:207-235 fuse), conv.py:91-108 DSConv pointwise+BN+SiLU,
 *                             nn.Conv2d 1x1 in Detect/LSKblock/DySample, nn.Linear in AdaHG
 *   ydbl_dsconv_nhwc       <- DSConv.forward conv.py:91-108 (dw + pw + BN + SiLU, one kernel)
 *   ydbl_dwconv2d_nhwc     <- depthwise nn.Conv2d (DSConv.dw conv.py:98, DWConv conv.py:128-133,
 *                             GhostConv.cv2 conv.py:194, LSKblock.conv0/conv_spatial LSKA.py:31-32)
 *   ydbl_dwconv2d_pair_nhwc<- LSKblock.forward LSKA.py:40-41 (conv0 -> conv_spatial, one launch)
 *   ydbl_letterbox         <- BasePredictor.preprocess engine/predictor.py:116-134 for ndarray frames:
 *                             LetterBox.__call__ data/augment.py:1535-1597 (cv2.resize INTER_LINEAR,
 *                             copyMakeBorder 114) + BGR->RGB + HWC->CHW + float /255
 *   ydbl_input_nchw_to_nhwc<- BasePredictor.preprocess engine/predictor.py:116-134 (+ LoadTensor /255)
 *   ydbl_conv_stem         <- preprocess (predictor.py:116-134) fused with the first backbone Conv
 *                             (conv.py:39-63 after fuse), reading the NCHW fp32 batch directly
 *   ydbl_bottleneck_nhwc   <- Bottleneck.forward nn/modules/block.py:355-357 (cv1 -> cv2 [+ x], both
 *                             Conv = conv.py:39-63 after fuse) as one kernel
 *   ydbl_conv_stem2        <- preprocess + the backbone's first two Convs (layers 0-1 of the DBL yamls:
 *                             Conv(3,C0,3,1) -> Conv(C0,2*C0,3,2), conv.py:39-63 after fuse), fp16
 *   ydbl_gate_add          <- FullPAD_Tunnel.forward nn/modules/block.py:1954-1956
 *   ydbl_channel_gate_add  <- A2C2f.forward block.py:1404-1405 (x + gamma * y)
 *   ydbl_area_attn         <- AAttn.forward block.py:1243-1264 (softmax(q^T k / sqrt(32)) v per area chunk)
 *   ydbl_psa_attn          <- Attention.forward block.py:919-928 (C2PSA / PSABlock: softmax(q^T k / sqrt(32)) v over
 *                             all tokens, key_dim 32, head_dim 64) without its convs
 *   ydbl_maxpool5_cascade  <- SPPF.forward block.py:194-198 (the three chained MaxPool2d(5, 1, 2))
 *   ydbl_pool_up_concat    <- FuseModule.forward block.py:1831-1840, DownsampleConv block.py:1927,
 *                             nn.Upsample(scale_factor=2, mode="nearest")
 *   ydbl_dysample(_ex)     <- DySample.sample modules_upsample/DySample.py:48-61 (grid_sample border)
 *   ydbl_dysample2         <- DySample.forward DySample.py:63-81 (offset conv + sample, one launch)
 *   ydbl_lsk_gate          <- LSKblock.forward LSKA.py:40-52 (mean/max, 7x7 squeeze, sigmoid gating)
 *   ydbl_lsk_attn/_out     <- LSKblock.forward LSKA.py:43-52 (conv1 | conv2 + stats; gate + conv + x *)
 *   ydbl_hg_*              <- AdaHyperedgeGen/AdaHGConv block.py:1627-1708 (ydbl_hg_fused: the whole
 *                             AdaHGConv incl. pre_head_proj block.py:1645, one call;
 *                             ydbl_hg_fused_pair: HyperACE's two C3AH branches block.py:1886-1895
 *                             in one set of launches)
 *   ydbl_detect_decode     <- Detect._inference head.py:143-181 + DFL block.py:79-83 +
 *                             make_anchors/dist2bbox utils/tal.py:333-357 + NMS candidate
 *                             filter utils/ops.py:234-276
 *   ydbl_detect_decode_aug <- the same for one pass of DetectionModel._predict_augment nn/tasks.py:361-398
 *                             (_descale_pred, _clip_augmented and the concatenation done as it writes)
 *   ydbl_scale_img         <- scale_img utils/torch_utils.py:423-432 (+ x.flip(3), nn/tasks.py:371)
 *   ydbl_pred_candidates   <- utils/ops.py:234-276 on a [B,4+nc,A] prediction tensor
 *   ydbl_nms               <- utils/ops.py:278-310 (+ torchvision.ops.nms, torchvision 0.23.0),
 *                             with clip_boxes utils/ops.py:319-338 as reached through
 *                             scale_boxes :92-127 for tensor sources (gain 1, pad 0)
 *   ydbl_nms (out_idx)     <- the row index `i` of utils/ops.py:300-310 (output[xi] = x[i]): which prediction row a kept
 *                             detection came from, so that its mask coefficients can be found afterwards
 *   ydbl_deconv2x2_nhwc    <- nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True) in Proto, nn/modules/block.py:87-104
 *   ydbl_process_mask      <- process_mask / process_mask_native utils/ops.py:661-713 with crop_mask :644-658 and
 *                             scale_masks :716-737 (F.interpolate bilinear, align_corners=False)
 *   ydbl_match_predictions <- DetectionValidator._process_batch models/yolo/detect/val.py:209-227
 *                             (box_iou utils/metrics.py:52-71 + BaseValidator.match_predictions
 *                             engine/validator.py:222-262, non-scipy branch)
 *   ydbl_gt_mask_bits      <- SegmentationValidator._process_batch(masks=True) models/yolo/segment/val.py:204-212
 *                             (the index map's indicator, F.interpolate bilinear, > 0.5), as bit planes
 *   ydbl_mask_iou          <- mask_iou utils/metrics.py:137-153 as segment/val.py:213 calls it, popcount on bit planes
 *   ydbl_match_iou         <- segment/val.py:217: match_predictions on the mask IoU matrix
 *   ydbl_pose_keypoints    <- Pose.kpts_decode nn/modules/head.py:396-401 for the rows the NMS kept, in fp32
 *   ydbl_kpt_oks           <- kpt_iou utils/metrics.py:156-175 with the label areas of models/yolo/pose/val.py:192
 *   ydbl_confusion_matrix  <- ConfusionMatrix.process_batch utils/metrics.py:326-382 and its call sites in
 *                             DetectionValidator.update_metrics models/yolo/detect/val.py:140-159
 *   ydbl_coco_match        <- COCOeval.evaluateImg (the COCO detection protocol's per-image, per-category greedy
 *                             matching) as DetectionValidator.eval_json reaches it,
 *                             models/yolo/detect/val.py:297-337; no crowd labels
 *   ydbl_global_avgpool    <- BaseModel._predict_once with embed set, nn/tasks.py:168-169
 *                             (adaptive_avg_pool2d(x, (1, 1)).squeeze(-1).squeeze(-1) of a layer's output)
 *   ydbl_bytetrack_update  <- BYTETracker.update trackers/byte_tracker.py:293-405 as driven per image by
 *                             on_predict_postprocess_end trackers/track.py:53-87
 *   ydbl_detect_loss       <- v8DetectionLoss.__call__ utils/loss.py:206-260 (BboxLoss :99-113, DFLoss :73-88,
 *                             bbox_iou CIoU utils/metrics.py:74-134) + TaskAlignedAssigner utils/tal.py:40-295,
 *                             forward only, as DetectionModel.loss nn/tasks.py:294-310 reaches it
 *   ydbl_detect_loss_grad  <- autograd's backward of the same call: BCE utils/loss.py:247, BboxLoss :99-113 with
 *                             bbox_decode :197-204, DFLoss :73-88, bbox_iou CIoU utils/metrics.py:102-130 (alpha
 *                             under no_grad :128-129); the assigner is a constant (utils/loss.py:233-243)
 */
#ifndef YDBL_H
#define YDBL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { YDBL_OK = 0, YDBL_EINVAL = 1, YDBL_ELAUNCH = 2, YDBL_ECAPACITY = 3 };
enum { YDBL_F32 = 0, YDBL_F16 = 1 };
enum { YDBL_ACT_NONE = 0, YDBL_ACT_SILU = 1, YDBL_ACT_GELU = 2, YDBL_ACT_SIGMOID = 3 };
enum { YDBL_RES_NONE = 0, YDBL_RES_ADD = 1, YDBL_RES_MUL = 2 };

typedef struct {
  void* ptr;  /* device pointer to element (0,0,0,0) of the view */
  int32_t n, h, w, c;
  int32_t cs; /* channel stride in elements (>= c) */
  int32_t dtype;
} ydbl_view;

/* Dense (groups = 1) convolution, implicit GEMM on MFMA (f16: 16x16x32, f32: exact 16x16x4).
 * y = act(conv(x, w) + bias); then res_mode ADD: y = r + y, MUL: y = r * y.
 * w: [cout][kh][kw][cin] in the view dtype, with cin == x.c (x.c must be a multiple of 8),
 *    rows padded to kpad = round_up(kh*kw*cin, 32) elements with zeros.
 * bias: fp32 [cout] or NULL.  r: view or NULL.
 * x.c, y.c multiples of 8 except y.c may be < 8 only when y.cs is a multiple of 4. */
typedef struct {
  ydbl_view x, y, r;
  const void* w;
  const float* bias;
  int32_t kh, kw, stride, pad, dil;
  int32_t kpad;
  int32_t act, res_mode;
  /* Optional second output, FullPAD_Tunnel (nn/modules/block.py:1954-1956) fused into the layer
   * that produces one of its inputs: y2 = a2 * v + b2 * r2, v = the value stored to y (rounded to
   * the view dtype first).  y2.ptr == NULL disables it; y2/r2 have y's shape and dtype. */
  ydbl_view y2, r2;
  float a2, b2;
  /* fp8 operands (f16 activations only): when dq != NULL, w holds OCP e4m3 bytes [cout][kpad]
   * quantized with per-output-channel scales sw, activations are quantized to e4m3 with
   * x * qscale (saturated to +-448) as they are staged, and dq[co] = 1 / (sw[co] * qscale)
   * dequantizes the fp32 accumulator before bias and activation. */
  const float* dq;
  float qscale;
  /* optional split-K scratch (fp32 partial tiles; f16 convs only): workspace_bytes >= ydbl_conv_workspace(d) lets the deep-K
   * wave-split-K path split its k-loop over up to 4 workgroups per tile when the map gives too few tiles to fill the
   * chip (the 20^2 / 40^2 maps of small sub-batches), the partials summed in fixed order by a second kernel that
   * runs the fused epilogue; NULL / too small: no split (same result up to the fp32 summation order) */
  void* workspace;
  int64_t workspace_bytes;
} ydbl_conv_desc;
int ydbl_conv2d_nhwc(const ydbl_conv_desc* d, void* stream);
/* ydbl_conv_workspace: the split-K scratch, in bytes, of the route this descriptor takes when it has all the room it
 * asks for (the environment switches as they are now); 0: that route does not split; -1: an invalid descriptor.
 * ydbl_conv_route: what ydbl_conv2d_nhwc would launch for this descriptor (its workspace as given, the switches as
 * they are now), without launching; YDBL_OK, or YDBL_EINVAL for an invalid descriptor or a NULL out.
 *   family  v[0..3]
 *   VW      Cin of the instance (128 or 64), output rows per tile        VGPR-weight 3x3 (conv3x3_vw_kernel)
 *   TILE    Cin, 16-channel output tiles, stride                         thin-input spatial tile (conv3x3_tile_kernel)
 *   HALO    stride, images per workgroup, channel-slice width (32 / 64)  halo 3x3 (conv3x3_halo_kernel)
 *   WSK     BM, BN                                                       wave-split-K (conv_wsk_kernel)
 *   IGEMM   BM, BN, WM, WN                                               block implicit GEMM (conv_igemm_kernel)
 * pointwise: the 1x1 / stride 1 / pad 0 instance.  ksplit > 1: a split-K launch followed by the epilogue kernel.
 * epi: the epilogue form compiled into the chosen instance, YDBL_ACT_SILU or YDBL_ACT_NONE; -1: the form that reads
 * the descriptor at run time; -2: the kernel picks the form itself, once per wave.  grid: the (first) kernel's grid.
 * workspace_bytes: ydbl_conv_workspace(d), whatever workspace the descriptor carries. */
enum { YDBL_CONV_VW = 0, YDBL_CONV_TILE = 1, YDBL_CONV_HALO = 2, YDBL_CONV_WSK = 3, YDBL_CONV_IGEMM = 4 };
typedef struct {
  int32_t family;
  int32_t v[4];
  int32_t pointwise;
  int32_t ksplit;
  int32_t epi;
  uint32_t grid[3];
  int64_t workspace_bytes;
} ydbl_conv_route_info;
int64_t ydbl_conv_workspace(const ydbl_conv_desc* d);
int ydbl_conv_route(const ydbl_conv_desc* d, ydbl_conv_route_info* out);

/* DSConv in one kernel (conv.py:91-108): y = act(pw(dw(x)) + bias) [+ r], BN folded into pw.
 * dw_w fp32 [k*k][cin], pw_w [cout][kpad] in the view dtype (kpad = round_up(cin, 32), zero
 * padded), bias fp32 [cout].  cin multiple of 32 (f16) / 16 (f32).  The depthwise output is
 * rounded to the view dtype (the reference's intermediate tensor) and never leaves LDS.
 * dw_bias (fp32 [cin] or NULL) and dw_act extend it to the Detect head's DWConv -> Conv1x1 pair
 * (head.py:93-101: dw = SiLU(BN(dwconv)), folded): dw output = dw_act(dw(x) + dw_bias). */
typedef struct {
  ydbl_view x, y, r;
  const float* dw_w;
  const void* pw_w;
  const float* bias;
  int32_t k, stride, pad, dil;
  int32_t kpad, act, res_mode;
  const float* dw_bias;
  int32_t dw_act;
  /* optional trailing 1x1 conv (Detect cls conv cv3[i][2], head.py:93-101) over y's 64 channels:
   * tail_y[p][k] = sum_c tail_w[k][c] * y[p][c] + tail_b[k], k < tail_n <= 4 (y is still written, unless
   * y_unused below) */
  const float* tail_w;
  const float* tail_b;
  ydbl_view tail_y;
  int32_t tail_n;
  /* optional NMS-candidate sink of the tail (cand_count != NULL; f16 only): the launch is one Detect level's class
   * branch (tail_n = nc) and appends that level's candidates to the lists of ydbl_decode_desc itself, exactly as
   * ydbl_detect_decode would from tail_y and box: same filter (conf_thres, multi_label, classes), same scores
   * (sigmoid of the stored f16 logit), same boxes, cand_idx = anchor (anchor * nc + cls when multi_label) with
   * anchor = anchor0 + y * w + x.  box: the level's DFL logits [n,h,w,64] (f16, 16-byte aligned), written by an
   * earlier launch of the stream and read only at pixels that hold a candidate.  level_stride: the level's stride.
   * zero_counts != 0: cand_count[0..n) is zeroed by a kernel of this call ahead of the tiles -- set it on the first
   * level's launch, clear it on the others, and the lists carry no state between calls.  Candidate order within an
   * image is free (ydbl_nms sorts by (score, cand_idx)). */
  float* cand_box;
  float* cand_score;
  int32_t* cand_cls;
  int32_t* cand_idx;
  int32_t* cand_count;
  int32_t cand_cap;
  float conf_thres;
  int32_t multi_label;
  int32_t nclasses;
  const int32_t* classes;
  float level_stride;
  int32_t anchor0;
  ydbl_view box;
  int32_t zero_counts;
  /* != 0 (tail only): nothing reads y, and the launch may leave it unwritten (the one-round-trip 64 -> 64 tile
   * does; y's shape fields still describe the map, its pointer must still be valid) */
  int32_t y_unused;
  /* optional deferred mode of the sink (tile_mask != NULL; needs cand_count): the level's box launch runs AFTER this
   * one, as ydbl_bottleneck_nhwc with the same tile_mask and a candidate sink, and computes box logits only where a
   * candidate is.  This launch filters, scores and takes slots exactly as above and writes cand_score, cand_cls and
   * cand_idx; it does not read box (the view is ignored) and does not write cand_box.  Instead it stores 1 into the
   * mask byte of each candidate's tile: tile_mask[(img * mask_tiles_img) + (y / 8) * mask_tiles_x + x / 16] -- the
   * mask granularity is the box kernel's tile, 8 rows x 16 columns, so mask_tiles_x = ceil(w / 16) and
   * mask_tiles_img = mask_tiles_x * ceil(h / 8) (checked).  mask_zero / mask_zero_bytes: one contiguous buffer holding
   * the masks of every deferred level of the head; the call that has zero_counts set zeroes it in the same kernel as
   * the counters (it need not have a tile_mask of its own), so no mask state is carried between calls. */
  uint8_t* tile_mask;
  int32_t mask_tiles_x;
  int32_t mask_tiles_img;
  uint8_t* mask_zero;
  int32_t mask_zero_bytes;
} ydbl_dsconv_desc;
int ydbl_dsconv_nhwc(const ydbl_dsconv_desc* d, void* stream);

/* Depthwise convolution (groups = C), fp32 arithmetic.
 * y = act(dwconv(x, w) + bias), then res_mode ADD: y = r + y (GhostBottleneck identity shortcut).
 * w: fp32 [kh][kw][c]; bias: fp32 [c] or NULL; r: view or ignored. */
typedef struct {
  ydbl_view x, y, r;
  const float* w;
  const float* bias;
  int32_t kh, kw, stride, pad, dil;
  int32_t act, res_mode;
} ydbl_dwconv_desc;
int ydbl_dwconv2d_nhwc(const ydbl_dwconv_desc* d, void* stream);

/* Two chained depthwise convs, d1.x == d0.y: LSKblock's conv0 (5x5) -> conv_spatial (7x7, dil 3)
 * (modules_attention/LSKA.py:40-41).  One launch with the whole map in LDS when H*W <= 512 (the P5
 * maps at 640), bit-identical to the two ydbl_dwconv2d_nhwc launches it falls back to otherwise.
 * fp16 without activation, pads 2 and 9, and both zero-padded maps ((H+4)(W+4) + (H+18)(W+18) pixels x 16
 * channels) within 80 KiB of LDS run a kernel that keeps the padded taps as fma(0, w, acc) terms instead of
 * skipping them: bit-identical for FINITE WEIGHTS (an infinite or NaN tap turns the padded border into NaN);
 * YDBL_DW_PAIR_OLD=1 (read per launch) keeps the tap-skipping kernel.
 * ydbl_dwconv2d_pair_route: what the call above would launch for these descriptors, without launching:
 * 0 the two ydbl_dwconv2d_nhwc launches, 1 the tap-skipping kernel, 2 the padded-map kernel; -1 a NULL descriptor. */
int ydbl_dwconv2d_pair_nhwc(const ydbl_dwconv_desc* d0, const ydbl_dwconv_desc* d1, void* stream);
int ydbl_dwconv2d_pair_route(const ydbl_dwconv_desc* d0, const ydbl_dwconv_desc* d1);

/* Input binding: the batch a graph-captured plan reads, chosen when the plan RUNS (YOLO.predict on a device tensor
 * without a staging copy).  When a kernel below gets a non-NULL `bind`, it takes the NCHW fp32 batch pointer from the
 * device word *bind->x (16-byte aligned, the same shape as x) and the scale from the device scalar *bind->amax, the
 * batch maximum, by LoadTensor's rule (U/data/loaders.py:561-566: x / 255 when max > 1 + FLT_EPSILON, else x; the
 * division is the multiply by fp32(1/255) that the GPU division computes) -- instead of x and scale.  A record
 * with both pointers NULL is no binding (x and scale are used); exactly one NULL is an error. */
typedef struct {
  const float* const* x; /* device word holding the batch pointer */
  const float* amax;     /* device fp32 scalar: the batch maximum */
} ydbl_input_bind;

/* The batch maximum of an input binding, on the device (LoadTensor's /255 decision, U/data/loaders.py:561-566), in
 * one launch: amax[0] = max of the n floats at x (16-byte aligned; NaN propagates as in torch.max) and, when scale
 * is not NULL, scale[0] = fp32(1/255) if amax > 1 + FLT_EPSILON else 1.  work: ydbl_batch_max_work_ints() int32
 * prepared by ydbl_batch_max_work_init (every call leaves them so); one work buffer per stream in flight. */
int32_t ydbl_batch_max_work_ints(void);
void ydbl_batch_max_work_init(int32_t* host_work);
int ydbl_batch_max(const float* x, int64_t n, int32_t* work, float* amax, float* scale, void* stream);
/* The same with the batch pointer read from the device word *xword when the launch runs (the first launch of a
 * captured predict graph, include/ydbl.h ydbl_input_bind); the batch must be 16-byte aligned. */
int ydbl_batch_max_bound(const float* const* xword, int64_t n, int32_t* work, float* amax, float* scale,
                         void* stream);

/* NCHW fp32 image batch -> NHWC view (channels >= 3 zero-filled up to y.cs), optional scale (1/255); bind: NULL or
 * the input binding above. */
int ydbl_input_nchw_to_nhwc(const float* x, int32_t n, int32_t c, int32_t h, int32_t w, float scale,
                            const ydbl_view* y, const ydbl_input_bind* bind, void* stream);

/* Stem: y = act(conv_kxk(x * scale) + bias) straight from an NCHW fp32 batch x [n][cin][h][w]
 * (cin = 3), w fp32 [cout][cin][k][k] (torch layout, BN folded), bias fp32 [cout]; y NHWC view with
 * y.c = cout (multiple of 4, <= 64); k = 3, pad = 1, stride 1 or 2.  In f16 mode the scaled input is rounded
 * to f16 before the conv (the reference's .half() input); arithmetic is fp32. */
int ydbl_conv_stem(const float* x, int32_t n, int32_t cin, int32_t h, int32_t w, float scale, const float* wt,
                   const float* bias, int32_t k, int32_t stride, int32_t act, const ydbl_view* y,
                   const ydbl_input_bind* bind, void* stream);

/* y = a + gate * b (FullPAD_Tunnel). */
int ydbl_gate_add(const ydbl_view* a, const ydbl_view* b, float gate, const ydbl_view* y, void* stream);

/* y = a + gate[c] * b, gate an fp32 device vector [c], 16-byte aligned (A2C2f's residual x + gamma * y). */
int ydbl_channel_gate_add(const ydbl_view* a, const ydbl_view* b, const float* gate, const ydbl_view* y,
                          void* stream);

/* AAttn's attention core (U/nn/modules/block.py:1243-1264), head_dim 32.
 * qkv: [n,h,w,3*C] NHWC view, C = heads*32, channel = head*96 + {q 0..31 | k 32..63 | v 64..95}.
 * The h*w tokens of an image, in row-major order, form `area` contiguous chunks of T = h*w/area tokens;
 * for each (image, chunk, head): P = softmax(q k^T * scale) over the chunk's T keys, y = P v.
 * y: [n,h,w,C] view, channel = head*32 + d.  v: the V part re-laid the same way (the input of AAttn.pe),
 * or a null view (ptr NULL) to skip it.  h*w % area != 0 is an error (the reference's reshape fails too).
 * Any T >= 1: key / value tiles stream through LDS with an online softmax.  f16: f16 MFMA, fp32 maximum, sum and
 * accumulators, P rounded to f16 for P v; f32: the fp32 MFMA.  All views 16-byte aligned channel vectors;
 * y and v must not overlap qkv.  n * area * heads <= 65535. */
typedef struct {
  ydbl_view qkv, y, v;
  int32_t heads, area;
  float scale;
} ydbl_area_attn_desc;
int ydbl_area_attn(const ydbl_area_attn_desc* d, void* stream);

/* C2PSA's attention core (Attention.forward without its convs, U/nn/modules/block.py:919-928), key_dim 32, head_dim 64.
 * qkv: [n,h,w,heads*128] NHWC view, channel = head*128 + {q 0..31 | k 32..63 | v 64..127} (the reference's
 * view(B, heads, 2*kd + hd, N).split -- not q | k | v by thirds).  For each (image, head): P = softmax(q k^T * scale)
 * over all N = h*w keys (scale = key_dim^-0.5 in the reference), y = P v.
 * y: [n,h,w,heads*64] view, channel = head*64 + d.  v: the V part re-laid the same way (the input of Attention.pe),
 * or a null view (ptr NULL) to skip it.  Any N >= 1: key / value tiles stream through LDS with an online softmax, tail
 * keys masked.  f16: f16 MFMA, fp32 maximum, sum and accumulators, P rounded to f16 for P v; f32: the fp32 MFMA.
 * All views 16-byte aligned channel vectors; y and v must not overlap qkv or each other.  key_dim and head_dim are
 * descriptor fields so that a caller states what it has: anything but 32 / 64 is YDBL_EINVAL.
 * Grid (query tile of 64, head, image): heads <= 65535, n <= 65535, h*w < 2^31, else YDBL_EINVAL. */
typedef struct {
  ydbl_view qkv, y, v;
  int32_t heads, key_dim, head_dim;
  float scale;
} ydbl_psa_attn_desc;
int ydbl_psa_attn(const ydbl_psa_attn_desc* d, void* stream);

/* SPPF's three cascaded max-pools (U/nn/modules/block.py:179-198) in one launch: y1 = m(x), y2 = m(y1), y3 = m(y2),
 * m = MaxPool2d(k, 1, k / 2) with -inf padding, computed as the 5x5, 9x9 and 13x13 windowed maxima of x clipped at the
 * border -- the same values exactly (a maximum never rounds; NaN propagates as in torch; the sign of a zero that ties
 * with the other zero is unspecified).  x, y1, y2, y3: [n,h,w,c] views of one shape and dtype, typically four channel
 * slices of SPPF's concat buffer (cs >= c), 16-byte aligned channel vectors; no output may overlap x or another
 * output.  k must be 5.  n <= 65535, c <= 131070 channel vectors, n*h < 2^31, else YDBL_EINVAL. */
typedef struct {
  ydbl_view x, y1, y2, y3;
  int32_t k;
} ydbl_maxpool5_desc;
int ydbl_maxpool5_cascade(const ydbl_maxpool5_desc* d, void* stream);

/* y[..., off0:] = avgpool2(p_lo); y[..., off1:] = p_mid; y[..., off2:] = nearest_up2(p_hi).
 * Any of p_lo / p_mid / p_hi may be NULL (DownsampleConv uses p_lo only). */
int ydbl_pool_up_concat(const ydbl_view* p_lo, const ydbl_view* p_mid, const ydbl_view* p_hi,
                        const ydbl_view* y, void* stream);

/* DySample 'lp' x2 sampling: off view [n,h,w,8*groups] in x's dtype (fp16 in half mode, as the reference's
 * .half() offset conv produces it) holding 0.25*offset+init_pos
 * (channel k = coord*4g + group*4 + i*2 + j), bilinear border grid_sample of x into y [n,2h,2w,c]. */
int ydbl_dysample(const ydbl_view* x, const ydbl_view* off, int32_t groups, const ydbl_view* y, void* stream);
/* Same, descriptor form with an optional second output (y2.ptr != NULL): y2 = a2 * y + b2 * r2 -- a
 * FullPAD_Tunnel (nn/modules/block.py:1954-1956) fed by this DySample, fused into its epilogue. */
typedef struct {
  ydbl_view x, off;
  int32_t groups;
  ydbl_view y, y2, r2;
  float a2, b2;
} ydbl_dysample_desc;
int ydbl_dysample_ex(const ydbl_dysample_desc* d, void* stream);
/* The whole DySample forward (DySample.py:48-81: offset conv + grid_sample) in one launch: off_w [8*groups][c]
 * in x's dtype holds the offset conv weights * 0.25 (K contiguous), off_b fp32 [8*groups] = 0.25 * bias +
 * init_pos (both folds exact); the offsets are rounded to x's dtype as the two-launch path stores them, and the
 * result is bit-identical to ydbl_conv2d_nhwc + ydbl_dysample_ex.  groups = 4, c / groups in {16, 32, 64}. */
typedef struct {
  ydbl_view x;
  const void* off_w;
  const float* off_b;
  int32_t groups;
  ydbl_view y, y2, r2;
  float a2, b2;
} ydbl_dysample2_desc;
int ydbl_dysample2(const ydbl_dysample2_desc* d, void* stream);

/* LSKblock gate: attn view = [a1 | a2] (2*half channels, each half = dim/2);
 * agg = [mean_c, max_c](attn); sig = sigmoid(conv7x7(agg) + sb); out = a1*sig0 + a2*sig1.
 * sw: fp32 [2][2][7][7] (torch layout), sb: fp32 [2]. */
int ydbl_lsk_gate(const ydbl_view* attn, const float* sw, const float* sb, const ydbl_view* out,
                  void* workspace, void* stream);
int64_t ydbl_lsk_gate_workspace(int32_t n, int32_t h, int32_t w);
/* LSKblock after its depthwise pair (LSKA.py:43-52) in two launches, fp16, dim in {256, 512}:
 *   ydbl_lsk_attn: attn = [conv1(a1) + b1 | conv2(a2) + b2] (w12 rows 0..dim/2-1 = conv1, the rest conv2,
 *                  each [dim/2][dim] K-contiguous fp16, b12 fp32 [dim]) and, per pixel, agg = [mean_c, max_c](attn)
 *                  (fp32 [n*h*w][2] in `agg`, the rounded attn reduced in ydbl_lsk_gate's order);
 *   ydbl_lsk_out:  y = x * (conv(a1' * sig0 + a2' * sig1) + b), sig = sigmoid(squeeze7x7(agg) + sb), w [dim][dim/2]
 *                  fp16 K-contiguous, b fp32 [dim] -- the gate never leaves the CU.
 * Bit-identical to ydbl_conv2d_nhwc (conv1, conv2) + ydbl_lsk_gate + ydbl_conv2d_nhwc (conv, RES_MUL) where
 * those run the block GEMM (dim 256).  a1, a2, attn, x, y: [n,h,w,dim] views (channel stride multiple of 8). */
typedef struct {
  ydbl_view x, a1, a2, attn, y;
  const void* w12;
  const float* b12;
  const float* sw;  /* conv_squeeze fp32 [2][2][7][7] */
  const float* sb;  /* [2] */
  const void* w;
  const float* b;
  float* agg;       /* ydbl_lsk_gate_workspace(n, h, w) bytes */
} ydbl_lsk_desc;
int ydbl_lsk_attn(const ydbl_lsk_desc* d, void* stream);
int ydbl_lsk_out(const ydbl_lsk_desc* d, void* stream);

/* Adaptive hypergraph (AdaHGConv), tokens = NHWC pixels of view x (D = x.c, N = h*w). */
typedef struct {
  ydbl_view x;      /* tokens X (input, also the residual) */
  ydbl_view xp;     /* pre_head_proj(X), produced by ydbl_conv2d_nhwc */
  ydbl_view y;      /* output: GELU(node_proj(A @ He)) + X */
  int32_t num_edges, num_heads;
  const float* proto_base;  /* [E][D] */
  const float* ctx_w;       /* [E*D][2D] (context 'both') */
  const float* ctx_b;       /* [E*D] */
  const float* edge_w;      /* [D][D] */
  const float* edge_b;      /* [D] */
  const float* node_w;      /* [D][D] */
  const float* node_b;      /* [D] */
  void* workspace;          /* ydbl_hg_workspace() bytes */
  const void* pre_w;        /* [D][D] pre_head_proj weight in x's dtype (ydbl_hg_fused only; else NULL) */
  const float* pre_b;       /* [D] pre_head_proj bias (ydbl_hg_fused only) */
} ydbl_hg_desc;
int64_t ydbl_hg_workspace(int32_t n, int32_t tokens, int32_t dim, int32_t edges);
/* stage 1: context stats + prototypes (run before the xp GEMM or after; independent of xp) */
int ydbl_hg_context(const ydbl_hg_desc* d, void* stream);
/* stage 2: logits, softmax over tokens, vertex->edge->vertex, residual (needs xp) */
int ydbl_hg_propagate(const ydbl_hg_desc* d, void* stream);
/* The whole AdaHGConv (block.py:1582-1708, pre_head_proj included: xp unused, pre_w/pre_b set) as five plain
 * kernels: three over (64-token slice, image) workgroups writing per-slice partials, two merging them (stream
 * order is the only synchronisation); head_dim 16, (dim, edges) in {64, 128} x {4, 8}.  workspace:
 * ydbl_hg_fused_workspace() bytes, uninitialised memory is fine; -1 = unsupported shape. */
int64_t ydbl_hg_fused_workspace(int32_t n, int32_t tokens, int32_t dim, int32_t edges, int32_t dtype);
int ydbl_hg_fused(const ydbl_hg_desc* d, void* stream);
/* ydbl_hg_fused(d0) followed by ydbl_hg_fused(d1), bit for bit, with both calls' workgroups in each of the five
 * launches (blockIdx.z picks the descriptor) when the two calls are independent and of one shape: both pass
 * ydbl_hg_fused's checks, agree in n, h*w, channels, num_edges, num_heads and dtype, neither y shares an element with
 * the other's x or y (channel slices of one buffer with disjoint ranges are fine), and the workspaces do not
 * intersect.  Otherwise the two calls run one after the other.  YDBL_EINVAL: a null descriptor. */
int ydbl_hg_fused_pair(const ydbl_hg_desc* d0, const ydbl_hg_desc* d1, void* stream);

/* Detect decode + NMS candidate extraction.
 * box[l]: fp32 view [n,h_l,w_l,64] (DFL logits), cls[l]: fp32 view [n,h_l,w_l,nc].
 * Writes, when y_ref != NULL, the reference output layout y[n][4+nc][A] (xywh pixels, sigmoid).
 * Candidates per image (cap each): xyxy boxes, score, class, original flat index
 * (anchor for single-label, anchor*nc+cls for multi-label); cand_count[n] (int32) is
 * zeroed by this call.  classes/ncls: optional class filter.  With y_ref == NULL the classes are evaluated first
 * and a box is decoded (its 64 logits read) only where a candidate is offered: same candidates, bit for bit. */
typedef struct {
  ydbl_view box[3], cls[3];
  int32_t nl, nc;
  float stride[3];
  float conf_thres;
  int32_t multi_label;
  const int32_t* classes; int32_t nclasses;
  float* y_ref;
  float* cand_box;     /* [n][cap][4] */
  float* cand_score;   /* [n][cap] */
  int32_t* cand_cls;   /* [n][cap] */
  int32_t* cand_idx;   /* [n][cap] */
  int32_t* cand_count; /* [n] */
  int32_t cap;
} ydbl_decode_desc;
int ydbl_detect_decode(const ydbl_decode_desc* d, void* stream);

/* One pass of test-time augmentation (DetectionModel._predict_augment, nn/tasks.py:361-398): ydbl_detect_decode of
 * a pass's head maps with the reference's _descale_pred and _clip_augmented applied as the values are written, so
 * that the three passes fill ONE prediction tensor y[n][4+nc][y_stride] and ONE candidate list, which a single
 * ydbl_nms then reads.  d is the pass's plain decode descriptor; the record below adds:
 *   scale     xywh are divided by it (IEEE fp32 division: torch's p[:, :4] /= scale; a reciprocal multiply differs
 *             on ~20 % of values); 0 = 1 = no de-scale
 *   flip_w    != 0: cx = flip_w - cx after the division (the left-right de-flip; flip_w = the input width)
 *   a_lo,a_hi the window [a_lo, a_hi) of the pass's own anchor order that survives _clip_augmented; anchors outside
 *             it are neither written to y_ref nor offered as candidates (a_hi = 0: every anchor)
 *   pos_base  position of anchor a_lo on the merged anchor axis: anchor a lands at pos = pos_base + (a - a_lo),
 *             y_ref column pos, and carries cand_idx = pos (pos * nc + cls when multi_label) -- ydbl_nms's
 *             (score desc, idx asc) order is then the reference's stable sort over the concatenation
 *   y_stride  row stride of y_ref in floats = the merged anchor count (0: the pass's own anchor count)
 *   append    nonzero: cand_count is NOT zeroed by this call (the first pass zeroes it, the later ones add);
 *             d->cap is the capacity of the shared list (the merged anchor count, x nc when multi_label)
 * The candidate boxes are xywh2xyxy of the de-scaled, de-flipped xywh, as the reference's NMS computes them from the
 * merged tensor.  An all-zero record is ydbl_detect_decode exactly. */
typedef struct {
  float scale;
  float flip_w;
  int32_t a_lo, a_hi;
  int32_t pos_base;
  int32_t y_stride;
  int32_t append;
} ydbl_decode_aug;
int ydbl_detect_decode_aug(const ydbl_decode_desc* d, const ydbl_decode_aug* g, void* stream);

/* NMS candidates straight from a prediction tensor in the reference layout
 * pred fp32 [n][4+nc][A] (xywh pixels, class scores), as U/utils/ops.py:234-276 reads it.
 * Same candidate outputs / semantics as ydbl_detect_decode. */
typedef struct {
  const float* pred;
  int32_t n, nc, A;
  float conf_thres;
  int32_t multi_label;
  const int32_t* classes; int32_t nclasses;
  float* cand_box; float* cand_score; int32_t* cand_cls; int32_t* cand_idx; int32_t* cand_count;
  int32_t cap;
} ydbl_pred_cand_desc;
int ydbl_pred_candidates(const ydbl_pred_cand_desc* d, void* stream);

/* Batched class-offset NMS over the candidates of ydbl_detect_decode.
 * out: fp32 [n][max_det][6] = x1,y1,x2,y2,conf,cls (kept, score order; rows past the count zeroed),
 * out_count int32 [n].  out_stride / count_stride (0 = dense): floats between images of out (>= max_det * 6)
 * and int32s between images of out_count -- e.g. one record per image [max_det*6 floats | count | pad], so
 * the boxes and counts of a batch-sharded predict travel in ONE all-gather (ydbl.parallel).
 * Semantics of U/utils/ops.py:278-310 + torchvision nms: candidates above max_nms are cut to the
 * max_nms highest scores; boxes offset by cls*max_wh (0 if agnostic); stable descending sort;
 * suppress j if IoU(i,j) > iou_thres (double compare); keep <= max_det.
 * clip_w/clip_h > 0: clamp kept boxes to [0,w]x[0,h] (scale_boxes with gain 1, pad 0).
 * per_image (schedule only, same output): 0 = the class-split sweep for non-agnostic NMS (one workgroup per image
 * and class group + a merge: the faster form when images carry thousands of candidates, e.g. validation's
 * conf 0.001); nonzero = one workgroup per image (the faster form when every image has at most 1024 candidates,
 * the pair-matrix path: predict's conf 0.25 -- DBL-n bs32 +0.8 %, profiles/r05/r05_nms_per_image_ab.txt). */
typedef struct {
  const float* cand_box; const float* cand_score; const int32_t* cand_cls; const int32_t* cand_idx;
  const int32_t* cand_count;
  int32_t n, cap;
  double iou_thres;
  int32_t max_det, max_nms, agnostic;
  float max_wh;
  float clip_w, clip_h;
  float* out; int32_t* out_count;
  void* workspace;
  int64_t out_stride, count_stride;
  int32_t per_image;
  /* optional int32 [n][max_det] (image stride max_det), NULL = not written: row k of image b receives the kept
   * candidate's cand_idx (anchor, or anchor * nc + cls in multi-label mode, as the decode wrote it), rows past the
   * count -1 -- what finds a detection's mask coefficients after the NMS (ydbl_process_mask) */
  int32_t* out_idx;
} ydbl_nms_desc;
int64_t ydbl_nms_workspace(int32_t n, int32_t cap, int32_t max_nms);
int ydbl_nms(const ydbl_nms_desc* d, void* stream);

/* The end2end (YOLOv10, v10Detect) head: no NMS, a top-k.
 *
 * ydbl_detect_decode_e2e: ydbl_detect_decode for a head with end2end = True (nn/modules/head.py:120-141, :196-198):
 * decode_bboxes calls dist2bbox(..., xywh=False), so a box is x1 = (ax - l) * stride, y1 = (ay - t) * stride,
 * x2 = (ax + r) * stride, y2 = (ay + b) * stride in fp32 and in that order of operations -- never xywh converted
 * back.  y_ref, when given, is the end2end layout [n][4+nc][A] with those xyxy rows; the candidate boxes are the same
 * four values.  Everything else (scores, filter, lists, counters) is ydbl_detect_decode's.
 *
 * ydbl_detect_topk: Detect.postprocess (head.py:200-221: the k anchors of largest best-class score, then the k largest
 * of their k * nc scores, k = min(max_det, A) with the head's own max_det = 300) followed by the six-column branch
 * of non_max_suppression (utils/ops.py:224-228: score > conf_thres, [:max_det], then the `classes` filter), over the
 * multi-label candidate lists of the decode (cand_idx = anchor * nc + cls, already thresholded by conf).  With
 * distinct scores the two chained topk's are the k largest of all (anchor, class) scores: a pair of an anchor outside
 * the first top-k has k pairs at least as large ahead of it.  Where scores tie torch.topk's order is unspecified;
 * OUR PINNED RULE is (score descending, cand_idx ascending), i.e. the smaller anchor, then the smaller class.
 * Per image: the first min(k_head, max_det) candidates in that order (k_head = min(head max_det, A), the caller's),
 * then, with classes != NULL, the rows whose class is not listed are dropped and the gaps closed, order kept -- the
 * filter comes after the cut, as in the reference.  iou, agnostic, multi_label, max_nms and max_wh play no part.
 * out / out_count, out_stride / count_stride and clip_w / clip_h: the contract of ydbl_nms_desc (rows
 * x1,y1,x2,y2,score,cls in selection order, rows past the count up to max_det zeroed, out_stride floats between
 * images), 1 <= max_det <= 4096.  cand_idx must be distinct within an image and scores positive (their bit patterns
 * then order like the values).  Nothing is sorted but the survivors: a radix select over 8-bit digits of the key
 * (score bits inverted | cand_idx) finds the k-th key, the <= k survivors are ranked in LDS.  per_image (schedule
 * only, same output): nonzero = one workgroup per image reads the list itself (predict thresholds: hundreds of
 * candidates); 0 = three launches ahead of it, split over the list (a chip-wide histogram of the score's exponent and
 * top mantissa bits, then a compaction of the bins that can hold a survivor), for validation's conf 0.001 and the
 * unthresholded A * nc candidates of DetectionModel.forward.  The histogram is summed with integer atomics and the
 * survivors are ordered by key, so the output is bit-identical from run to run.  workspace: caller-owned,
 * ydbl_detect_topk_workspace(n, cap) bytes, uninitialised memory is fine. */
int ydbl_detect_decode_e2e(const ydbl_decode_desc* d, void* stream);
typedef struct {
  const float* cand_box; const float* cand_score; const int32_t* cand_cls; const int32_t* cand_idx;
  const int32_t* cand_count;
  int32_t n, cap;
  int32_t k_head, max_det;
  const int32_t* classes; int32_t nclasses;
  float clip_w, clip_h;
  float* out; int32_t* out_count;
  int64_t out_stride, count_stride;
  void* workspace; int64_t workspace_bytes;
  int32_t per_image;
} ydbl_topk_desc;
int64_t ydbl_detect_topk_workspace(int32_t n, int32_t cap);
int ydbl_detect_topk(const ydbl_topk_desc* d, void* stream);

/* Stem pair (fp16): y = SiLU(conv3x3_s2(SiLU(conv3x3_s1(x * scale) + b0)) + b1), NHWC [n][ceil(h/2)][ceil(w/2)][2*c0],
 * from the NCHW fp32 batch x [n][3][h][w]; the full-resolution intermediate never leaves LDS.
 * params: device blob of ydbl_conv_stem2_params_size(c0) bytes filled on the HOST by
 * ydbl_conv_stem2_pack from fp32 weights w0 [c0][3][3][3], b0 [c0], w1 [2*c0][c0][3][3], b1 [2*c0]
 * (BN already folded); c0 = 8 or 16.  The first conv's bias enters the MFMA as an fp16 weight on a constant-1 input
 * slot (the reference's .half() bias), the second conv's is added in fp32. */
typedef struct {
  const float* x;
  int32_t n, cin, h, w;
  float scale;
  int32_t c0;
  const void* params;
  ydbl_view y;
  ydbl_input_bind bind; /* {NULL, NULL}: read x / scale */
} ydbl_stem2_desc;
int64_t ydbl_conv_stem2_params_size(int32_t c0);
int ydbl_conv_stem2_pack(const float* w0, const float* b0, const float* w1, const float* b1, int32_t c0, void* out);
int ydbl_conv_stem2(const ydbl_stem2_desc* d, void* stream);

/* Fused Bottleneck (fp16): y = [x +] SiLU(conv3x3(SiLU(conv3x3(x) + b1)) + b2), c -> c/2 -> c channels,
 * stride 1, pad 1 (Bottleneck(c, c, shortcut, e=0.5) with Conv = conv + folded BN + SiLU); the c/2
 * intermediate never leaves LDS.  x, y: NHWC fp16 views of the same shape with x.c == y.c == c
 * (c = 16, 32 or 64), y must not alias x.  params: device blob of ydbl_bottleneck_params_size(c)
 * bytes filled on the HOST by ydbl_bottleneck_pack from fp32 w1 [c/2][c][3][3], b1 [c/2],
 * w2 [c][c/2][3][3], b2 [c] (BN folded).  tile_h: 0 = auto, else 8 or 16 output rows per workgroup (or 9 for
 * c 64 / c_mid 32). */
typedef struct {
  ydbl_view x, y;
  int32_t c;
  int32_t add;
  int32_t tile_h;
  const void* params;
  int32_t c_mid;     /* intermediate channels: 0 = c/2 (Bottleneck e=0.5); 64 with c = 64 (Detect box branch) */
  int32_t pw;        /* 1: params from ydbl_detect_box_pack, y = conv1x1(cv2 output) + b3 (c = c_mid = 64) */
  /* optional sparse box launch (pw = 1 and 8-row tiles only, else YDBL_EINVAL).  tile_mask != NULL: one byte per
   * 8-row x 16-column tile, [n][ceil(h / 8)][ceil(w / 16)] (the deferred class tail of ydbl_dsconv_desc writes it); a
   * workgroup whose byte is 0 returns before it loads anything and leaves its part of y unwritten, the others compute
   * and store their tile exactly as the unmasked launch does.  cand_count != NULL (needs tile_mask): the candidate
   * sink -- after storing its tile a workgroup scans cand_idx[img][0 .. min(cand_count[img], cand_cap)), and for each
   * entry whose anchor (cand_idx, or cand_idx / nc when multi_label) lies in this level (anchor0 .. anchor0 + h*w) and
   * in its tile, decodes the box from the 64 logits as stored in f16 (DFL, dist2bbox, xywh2xyxy, level_stride: the
   * arithmetic of ydbl_detect_decode, bit for bit) into cand_box[img][slot].  1 <= nc <= 4. */
  const uint8_t* tile_mask;
  float* cand_box;
  const int32_t* cand_idx;
  const int32_t* cand_count;
  int32_t cand_cap;
  float level_stride;
  int32_t anchor0;
  int32_t nc;
  int32_t multi_label;
} ydbl_bottleneck_desc;
int64_t ydbl_bottleneck_params_size(int32_t c);
int ydbl_bottleneck_pack(const float* w1, const float* b1, const float* w2, const float* b2, int32_t c, void* out);
/* Same kernel for any (c, c_mid) pair it is built for -- (16,8) (32,16) (64,32) (64,64): two chained
 * 3x3 stride-1 Conv+SiLU, c -> c_mid -> c.  (64,64) replaces the Detect head's box-branch
 * cv2[i][0] -> cv2[i][1] (nn/modules/head.py:86-90) at 64 channels. */
int64_t ydbl_conv3x3_pair_params_size(int32_t c, int32_t c_mid);
int ydbl_conv3x3_pair_pack(const float* w1, const float* b1, const float* w2, const float* b2, int32_t c,
                           int32_t c_mid, void* out);
/* Detect box branch of one level, cv2[i] = Conv3x3(c_in,64) -> Conv3x3(64,64) -> Conv2d 1x1(64,64)+bias
 * (nn/modules/head.py:86-90), as one launch: desc.c = desc.c_mid = 64, desc.pw = 1, x.c = c_in in {64, 128}. */
int64_t ydbl_detect_box_params_size(int32_t c_in, int32_t c);
int ydbl_detect_box_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                         const float* b3, int32_t c_in, int32_t c, void* out);
int ydbl_bottleneck_nhwc(const ydbl_bottleneck_desc* d, void* stream);

/* LetterBox a batch of HWC uint8 BGR frames into one fp32 NCHW RGB canvas batch (values /255).
 * src: frames back to back, frame i at src + src_off[i] (int64 device array);
 * meta int32 device array [n][6] = (h, w, unpad_h, unpad_w, top, left) as LetterBox computes them
 * on the host; out fp32 [n][3][out_h][out_w]; pad_value is the border colour (114).
 * Resize = OpenCV 4.x uint8 INTER_LINEAR (see letterbox.hip for the exact fixed-point rules). */
typedef struct {
  const uint8_t* src; const int64_t* src_off; const int32_t* meta;
  int32_t n, out_h, out_w;
  float pad_value;
  float* out;
} ydbl_letterbox_desc;
int ydbl_letterbox(const ydbl_letterbox_desc* d, void* stream);

/* scale_img of test-time augmentation (utils/torch_utils.py:423-432) with the source's left-right flip folded in:
 * y[:, :, :sh, :sw] = bilinear resize (F.interpolate align_corners=False, no antialias; torch's fp32 source-index
 * rule, see scale_img.hip) of x (flip: of x.flip(3)) to (sh, sw); the rest of y [n][c][hp][wp] = pad_value (the
 * reference pads right and bottom with 0.447).  x fp32 [n][c][h][w], both dense; sh <= hp, sw <= wp.  The resize
 * ratio is implied by (sh, sw): the caller computes sh = int(h * ratio), hp = ceil(h * ratio / gs) * gs. */
typedef struct {
  const float* x;
  int32_t n, c, h, w;
  int32_t sh, sw;    /* resized extent */
  int32_t hp, wp;    /* padded output extent */
  int32_t flip;      /* nonzero: read the source mirrored left-right */
  float pad_value;
  float* y;
} ydbl_scale_img_desc;
int ydbl_scale_img(const ydbl_scale_img_desc* d, void* stream);

/* mAP true-positive matrix of a batch of NMS outputs against ground-truth labels.
 * det fp32 [n][max_det][6] (x1,y1,x2,y2,conf,cls) + det_count int32 [n] (ydbl_nms outputs);
 * labels grouped by image: gt_box fp32 [n_gt][4] xyxy, gt_cls fp32 [n_gt], gt_ofs int32 [n+1]
 * (image b owns labels gt_ofs[b] .. gt_ofs[b+1]-1, gt_ofs[n] == n_gt, original order kept);
 * iouv fp32 [n_iou] thresholds; single_cls: detections count as class 0.
 * correct uint8 [n][max_det][n_iou]: 1 where the detection is a TP at that IoU threshold
 * (rows >= det_count are zeroed).  Bit-exact with the reference for distinct IoUs; an exact IoU
 * tie between two same-class labels of one detection resolves to the larger label index. */
typedef struct {
  const float* det; const int32_t* det_count;
  int32_t n, max_det;
  const float* gt_box; const float* gt_cls; const int32_t* gt_ofs;
  int32_t n_gt;
  const float* iouv; int32_t n_iou;
  int32_t single_cls;
  uint8_t* correct;
  void* workspace; /* ydbl_match_workspace(n, max_det, n_gt, n_iou) bytes */
} ydbl_match_desc;
int64_t ydbl_match_workspace(int32_t n, int32_t max_det, int32_t n_gt, int32_t n_iou);
int ydbl_match_predictions(const ydbl_match_desc* d, void* stream);

/* Detection confusion matrix of a batch of NMS outputs against ground-truth labels, added into `matrix`:
 * ConfusionMatrix.process_batch (utils/metrics.py:326-382) as DetectionValidator.update_metrics calls it per image
 * (models/yolo/detect/val.py:140-159), with box_iou (utils/metrics.py:52-71) bitwise as ydbl_match_predictions
 * evaluates it.  det / det_count / gt_box / gt_cls / gt_ofs as in ydbl_match_desc; classes are truncated to int
 * like the reference's .int().  Row = predicted class, column = true class, index nc = background.  Per image:
 *   kept detections: rows d < min(det_count, max_det) with det[d][4] > (float)conf;
 *   a (label, detection) pair takes part when iou > (float)iou_thres (both compares strict, fp32);
 *   best(d)   = the label with the largest participating IoU of detection d,
 *   winner(l) = the detection with the largest iou(best(d), d) among those with best(d) == l;
 *   label l with a winner: matrix[cls(winner(l))][cls(l)] += 1, without one: matrix[nc][cls(l)] += 1;
 *   every kept detection that is no label's winner: matrix[cls(d)][nc] += 1.
 * This is what the reference's two argsort / np.unique passes select.  Our rule on exact IoU ties: the larger
 * label index wins best(d), the larger detection index wins winner(l) -- the order numpy's reversed argsort
 * gives for match arrays of up to 16 rows (above that numpy's own order on ties is unspecified).
 * A class outside [0, nc) on either side (the reference raises IndexError) writes nothing: that count is
 * skipped and *invalid is incremented.  matrix int64 [(nc+1)][(nc+1)] and invalid int32 [1] are accumulated
 * into (integer atomics: the result does not depend on scheduling); the caller zeroes them once per run.
 * conf in any range, iou_thres >= 0, 1 <= nc <= 32767, max_det <= 2^20; workspace 8-byte aligned. */
typedef struct {
  const float* det; const int32_t* det_count;
  int32_t n, max_det;
  const float* gt_box; const float* gt_cls; const int32_t* gt_ofs;
  int32_t n_gt;
  int32_t nc;
  float conf, iou_thres;
  int64_t* matrix;
  int32_t* invalid;
  void* workspace; /* ydbl_confusion_workspace(n, max_det, n_gt) bytes */
} ydbl_confusion_desc;
int64_t ydbl_confusion_workspace(int32_t n, int32_t max_det, int32_t n_gt);
int ydbl_confusion_matrix(const ydbl_confusion_desc* d, void* stream);

/* COCO-protocol matching of a batch of NMS outputs against ground-truth labels: what COCOeval.evaluateImg computes
 * per (image, category, area range), for every IoU threshold, without crowd labels.  det / det_count / gt_box /
 * gt_cls / gt_ofs as in ydbl_match_desc; a class is truncated to int and belongs to no category outside [0, nc);
 * single_cls: every detection and label is category 0.  iou_thrs fp64 [n_iou <= 16] and area_rng fp64 [n_area <= 8][2]
 * are HOST arrays, read during the call.
 * Boxes: x = x1, y = y1, w = x2 - x1, h = y2 - y1 after conversion to fp64; area = w * h; IoU, in fp64 without
 * contraction: iw = min(dx+dw, gx+gw) - max(dx, gx), ih likewise, 0 if iw <= 0 or ih <= 0, else
 * i = iw*ih, iou = i / (dw*dh + gw*gh - i).
 * Per (image, category): the rows d < min(det_count, max_det) of that category ordered by score descending (ties in
 * row order; a NaN score sorts last), cut to the first min(max_dets, max_det).  Per area range a = (a0, a1) and
 * threshold t: a label is ignored when its area < a0 or > a1; the detections, in that order, each take the label not
 * yet taken (for this a, t) with the largest IoU among those with iou >= min(t, 1 - 1e-10), a non-ignored label before
 * any ignored one, on an exact IoU tie the label later in label order; a matched detection inherits the label's
 * ignore flag, an unmatched one is ignored when its own area lies outside the range.
 * Outputs, each word written once by a plain vector store (no atomics on global memory; deterministic):
 *   dt_rank    int32 [n][max_det]          the row's position in its (image, category) list, or -1: a row past the
 *                                          count, of no category, or beyond the cut;
 *   dt_matched int32 [n][max_det][n_area]  bit t set: matched at iou_thrs[t] (0 where dt_rank is -1);
 *   dt_ignored int32 [n][max_det][n_area]  bit t set: ignored at iou_thrs[t] (0 where dt_rank is -1);
 *   gt_ignore  uint8 [n_gt][n_area]        the label's ignore flag (every label, whatever its class);
 *   invalid    int32 [n]                   rows below the count whose class is outside [0, nc) (0 with single_cls).
 * One launch: a workgroup per (category, image).  No allocation, no host sync, graph-capturable, reentrant.
 * ydbl_coco_workspace: bytes of `workspace` (0 today: the state is in LDS, and workspace may then be NULL; -1 for a
 * negative argument).  YDBL_EINVAL: null descriptor / pointer, n or max_det < 1, n > 65535, max_det > 2^20, nc outside
 * [1, 32767], n_iou outside [1, 16], n_area outside [1, 8], max_dets outside [1, 1024], a NaN threshold, an area range
 * with lo > hi.  YDBL_ECAPACITY: min(max_dets, max_det) detections and n_gt labels (all of which one image and category
 * may own) need more than the 160 KiB of LDS of a workgroup: 36 bytes per detection, 48 per label (100 detections
 * leave room for 3336 labels per batch).  Both are returned before any launch. */
typedef struct {
  const float* det; const int32_t* det_count;
  int32_t n, max_det;
  const float* gt_box; const float* gt_cls; const int32_t* gt_ofs;
  int32_t n_gt;
  int32_t single_cls;
  int32_t nc;
  const double* iou_thrs; int32_t n_iou;   /* host */
  const double* area_rng; int32_t n_area;  /* host, [n_area][2] */
  int32_t max_dets;                        /* the cut per (image, category): 100 */
  int32_t* dt_rank; int32_t* dt_matched; int32_t* dt_ignored;
  uint8_t* gt_ignore;
  int32_t* invalid;
  void* workspace; /* ydbl_coco_workspace(n, max_det, n_gt, nc) bytes */
} ydbl_coco_desc;
int64_t ydbl_coco_workspace(int32_t n, int32_t max_det, int32_t n_gt, int32_t nc);
int ydbl_coco_match(const ydbl_coco_desc* d, void* stream);

/* Global average pool of an NHWC view: y[n][c] = mean over (h, w) of x[n][.][.][c], the pooled layer feature of
 * BaseModel._predict_once with embed set (nn/tasks.py:168-169: adaptive_avg_pool2d(x, (1, 1)).squeeze(-1).squeeze(-1)).
 * fp32 accumulation, mean = sum / float(h*w) in fp32, one round-to-nearest-even to x's dtype.  Deterministic: no
 * floating-point atomics; the pixels of an image are cut into chunks by (h*w, c, dtype) alone -- never by n -- and
 * added in a fixed order, so image i's row has the same bits pooled alone, inside any batch and on every run.
 * More than one chunk per image: the chunks' fp32 partial rows go through `workspace` and a second launch on the same
 * stream adds them (ydbl_global_avgpool_workspace(d) bytes, 0 for a map of one chunk; 4-byte aligned; -1 for a
 * descriptor ydbl_global_avgpool would reject for its view).  x may be a channel slice (cs >= c, any element offset):
 * 16-byte loads when c, cs and the pointer allow them (multiples of 8 halves / 4 floats), else a scalar path --
 * never YDBL_EINVAL for alignment.  n <= 65535.  YDBL_EINVAL: null descriptor / x.ptr / y, empty view, bad dtype,
 * y_stride < c, workspace NULL or too small when one is needed.  No allocation, graph-capturable, reentrant. */
typedef struct {
  ydbl_view x;            /* NHWC view (channel slice allowed: cs >= c, any offset), YDBL_F16 or YDBL_F32 */
  void* y;                /* row n at y + n * y_stride elements, c elements, in x's dtype */
  int64_t y_stride;       /* elements; >= x.c (so several layers share one [B, D] row) */
  void* workspace;        /* fp32 partial sums, >= ydbl_global_avgpool_workspace(d) bytes; may be NULL when that is 0 */
  int64_t workspace_bytes;
} ydbl_avgpool_desc;
int64_t ydbl_global_avgpool_workspace(const ydbl_avgpool_desc* d);
int ydbl_global_avgpool(const ydbl_avgpool_desc* d, void* stream);

/* ByteTrack association of a batch of NMS outputs, on the device (BYTETracker.update trackers/byte_tracker.py:293-405
 * with STrack :51-228, KalmanFilterXYAH trackers/utils/kalman_filter.py:52-236, iou_distance / fuse_score /
 * linear_assignment trackers/utils/matching.py:20-157, and the per-image driver trackers/track.py:53-87).
 * det fp32 rows x1,y1,x2,y2,conf,cls and det_count int32 as ydbl_nms writes them; det_stride / count_stride (0 =
 * dense): floats between the images of det (>= max_det * 6) and int32s between the images of det_count, so the
 * records of ydbl_nms_desc (out_stride / count_stride) are read in place.  A count above max_det is clamped.
 * hw fp32 [n][2]: each image's (height, width), the extents the output boxes are clipped to.
 * One workgroup per tracker.  trackers == 1: the n images go through ONE tracker in row order, as consecutive frames
 * (the reference for every non-stream source); trackers == n: image i is the next frame of tracker i.  Anything else
 * is YDBL_EINVAL.  reset_each != 0: the tracker is reset before every image (persist=False).
 * Per image: out fp32 [n][max_det][7] rows x1,y1,x2,y2,id,conf,cls = the activated tracked tracks in the reference's
 * list order, clipped (rows past the count zeroed); out_count int32 [n]; tracked int32 [n] = 1 when rows were
 * written, 0 = "leave this image's predicted boxes as they are" (no detection: update() is not called and the
 * frame counter stays; or update() returned no track); out_idx int32 [n][max_det] or NULL: each row's detection
 * index (-1 past the count).
 * state: trackers * ydbl_bytetrack_state_bytes(max_tracks, max_det) bytes, 16-byte aligned, caller-owned, zeroed by
 * the caller: a zeroed state is a reset tracker.  Per tracker: int64 sequence counter | int32 frame_id, next id
 * (ids issued so far), overflow, slot high-water mark, 2 x pad | per slot mean[8] and cov[8][8] fp64, an int64
 * sequence key (list order), state, is_activated, id, frame_id, start_frame, tracklet_len, idx, removed-list
 * membership, score, cls.  More than max_tracks live tracks (tracked + lost + unconfirmed): no track is started for
 * that detection, no id is spent and `overflow` is incremented; nothing is overwritten.
 * Kalman arithmetic fp64, IoU and fused cost fp32 in numpy's operation order, score comparisons fp32.  The
 * assignment is exact: an optimum of sum_matched (c_ij - thresh) over the pairs with c_ij <= thresh (what
 * lap.lapjv(extend_cost=True, cost_limit=thresh) minimises), by shortest augmenting paths in fp64; where the optimum
 * is not unique the choice is unspecified.  Detections with a non-finite box, score or class, or of zero height,
 * take no part (never matched, never a new track).  The reference's removed_stracks list is kept as a per-slot
 * flag and is not cut at 1000 entries.  No allocation, no host sync, graph-capturable.
 * YDBL_EINVAL: null descriptor / pointer, n, max_det or max_tracks < 1, trackers not in {1, n}, a threshold outside
 * [0, 1], a stride too small, state too small or misaligned; YDBL_ECAPACITY: max_tracks and max_det together need
 * more than the 160 KiB of LDS of a workgroup (512 and 300 need 61 KiB). */
typedef struct {
  const float* det; const int32_t* det_count;
  int32_t n, max_det;
  int64_t det_stride, count_stride;
  const float* hw;
  double track_high_thresh, track_low_thresh, new_track_thresh, match_thresh;
  int32_t fuse_score, track_buffer;
  int32_t max_time_lost;   /* int(frame_rate / 30 * track_buffer), frame_rate 30 */
  int32_t max_tracks;
  int32_t trackers, reset_each;
  float* out; int32_t* out_count; int32_t* tracked; int32_t* out_idx;
  void* state;
  int64_t state_bytes;
} ydbl_track_desc;
int64_t ydbl_bytetrack_state_bytes(int32_t max_tracks, int32_t max_det); /* per tracker; -1: an argument < 1 */
int ydbl_bytetrack_update(const ydbl_track_desc* d, void* stream);

/* The detection loss of a batch, forward only: v8DetectionLoss.__call__ (utils/loss.py:206-260) with bbox_decode
 * (:197-204), BboxLoss (:99-113), DFLoss (:73-88), bbox_iou(CIoU=True) (utils/metrics.py:74-134) and the
 * TaskAlignedAssigner (utils/tal.py:40-295; alpha 0.5, beta 6.0, eps 1e-9; make_anchors :333-345, bbox2dist :360-363),
 * read from the Detect head's level buffers in place.  box[l] / cls[l]: the 64 box logits and the nc class logits of
 * level l as NHWC views (channel slices of one [B,h,w,64+nc] buffer or separate; YDBL_F16 or YDBL_F32, any channel
 * pitch, element-aligned); all arithmetic is fp32.  stride[l]: the level's stride; reg_max must be 16.
 * gt fp32 [B][max_labels][5]: rows cls, x1, y1, x2, y2 in input pixels, zero-padded; a row whose four box values sum
 * to <= 0 is padding (the reference's mask_gt).  A class is truncated to int and clamped into [0, nc): the caller
 * validates it.
 * The assignment: per label the `topk` (1..16; the reference: 10) anchors of largest align_metric =
 * sigmoid(class logit)^0.5 * max(CIoU, 0)^6 (CIoU of the label and predicted box * stride, in pixels) among the
 * anchors whose centre lies strictly inside the label's box (> 1e-9 on all four deltas), an equal metric going to
 * the lower anchor index.  A ZERO METRIC IS NOT SELECTED: the reference's topk, short of positive metrics, fills up
 * with zero-metric anchors in an order torch leaves unspecified; inside the box those become fg with target score 0
 * and weight 0 and change none of the three sums (fg / target_gt_idx may differ from the reference only there).
 * An anchor selected by more than one label goes to the argmax of the overlaps over ALL the image's labels (0 outside
 * a box and for padding; first index on ties), also to one that did not select it (tal.py:284-292).  The per-label
 * maxima of metric and overlap are taken after that, and target score = metric * max_overlap / (max_metric + 1e-9).
 * Box and DFL terms in grid units (label / stride), DFL target clamped to [0, 14.99], BCE over every anchor and class.
 * Outputs (each word written once; no floating-point atomics -- integer atomics for the pick counts, atomicMax on
 * the bits of non-negative floats for the maxima -- so all of them are bit-identical from run to run):
 *   loss fp32 [3]            box, cls, dfl: gain * sum / target_scores_sum (box and dfl 0 when nothing is fg);
 *   target_scores_sum fp32   max(sum of target scores, 1);
 *   per_image fp32 [B][3]    the same three sums restricted to one image, over the batch's target_scores_sum;
 *   fg int32 [B][A], target_gt_idx int32 [B][A], target_score fp32 [B][A]: optional (NULL: not written), the
 *                            assignment; target_score is the value that lands on the label's class.
 * A = sum of h*w over the levels, anchors in level order, row-major.  Five launches on `stream`; no allocation, no
 * host sync, graph-capturable, reentrant.  workspace: ydbl_detect_loss_workspace(B, A, max_labels) bytes, 16-byte
 * aligned (-1 for an argument < 1, max_labels < 0).  YDBL_EINVAL: null descriptor / buffer, nl outside 1..3, nc < 1,
 * reg_max != 16, topk outside 1..16, level shapes that disagree, B or max_labels > 65535, B*A*4 >= 2^31, workspace
 * too small or misaligned. */
typedef struct {
  ydbl_view box[3], cls[3];
  int32_t nl, nc, reg_max;
  float stride[3];
  const float* gt;
  int32_t max_labels;
  int32_t topk;
  float gain_box, gain_cls, gain_dfl;   /* hyp.box / cls / dfl: 7.5 / 0.5 / 1.5 (cfg/default.yaml:99-101) */
  float* loss; float* target_scores_sum; float* per_image;
  int32_t* fg; int32_t* target_gt_idx; float* target_score;
  void* workspace;
  int64_t workspace_bytes;
} ydbl_loss_desc;
int64_t ydbl_detect_loss_workspace(int32_t n, int32_t anchors, int32_t max_labels);
int ydbl_detect_loss(const ydbl_loss_desc* d, void* stream);

/* The gradient of the detection loss: d(loss.sum() * batch_size) / d(level logits) as the reference's autograd
 * defines it for v8DetectionLoss.__call__ (utils/loss.py:206-260), given the assignment ydbl_detect_loss wrote.  The
 * assigner's outputs are constants there -- it runs under torch.no_grad() on detached inputs (:233-243) -- so fg,
 * target_gt_idx, target_score and target_scores_sum are inputs here and receive no gradient, nor do the labels.
 * box / cls / nl / nc / reg_max / stride / gt / max_labels / gains: as in ydbl_loss_desc, the same buffers.
 * With S = target_scores_sum, K = (grad_scale ? *grad_scale : 1) * batch_scale (batch_scale: the reference's
 * `* batch_size`, :260; grad_scale: a device fp32 scalar, the upstream gradient of the total), and for a foreground
 * anchor w = target_score and the label gt[b][target_gt_idx]:
 *   class logits, every anchor and class (BCEWithLogitsLoss, :247): K * gain_cls / S * (sigmoid(x) - t), t = w on
 *     the label's class of a foreground anchor, 0 elsewhere;
 *   box logits of an anchor that is not foreground: 0 (written; the logits are not read);
 *   box logits of a foreground anchor, per side s of l, t, r, b with p = softmax over the side's 16 bins and
 *     d_s = sum j * p_j (bbox_decode, :197-204):
 *       K * gain_box / S * w * (-dCIoU/dd_s) * p_j * (j - d_s)                      (BboxLoss, :99-106)
 *     + K * gain_dfl / S * w / 4 * (p_j - wl * [j == tl] - wr * [j == tl + 1])        (DFLoss, :73-88, :107-109)
 *     The CIoU is bbox_iou(xywh=False, CIoU=True) (utils/metrics.py:102-130) of the predicted box (ax - d_l, ay - d_t,
 *     ax + d_r, ay + d_b) and label / stride, eps = 1e-7 on h1, h2, union and c2; ALPHA IS A CONSTANT (computed
 *     under torch.no_grad(), :128-129); the gradient passes through v and through the min / max / clamp(0)
 *     selections (a tie takes one side).  The DFL target is bbox2dist clamped to [0, 14.99], tl its integer part.
 * gbox[l] / gcls[l]: output views of the shapes of box[l] / cls[l], YDBL_F16 or YDBL_F32 independently of the inputs,
 * any channel pitch; lanes between c and the pitch are not touched.  All arithmetic is fp32, K included, and a value
 * is rounded once, to the output view's dtype (a loss scale in grad_scale therefore keeps the small fp16 gradients).
 * Every output word is written exactly once, no atomics: bit-identical from run to run and across pitches.  A whole
 * group of 8 channels moves as 16-byte accesses at element alignment (any pitch), the nc % 8 tail element by element.
 * One launch on `stream`; no allocation, no workspace, no host sync, graph-capturable, reentrant.  YDBL_EINVAL: as
 * ydbl_detect_loss for the shared fields, a null assignment buffer, a null gradient view or one whose shape differs
 * from its input's, B * A >= 2^31. */
typedef struct {
  ydbl_view box[3], cls[3];
  int32_t nl, nc, reg_max;
  float stride[3];
  const float* gt;
  int32_t max_labels;
  float gain_box, gain_cls, gain_dfl;
  const int32_t* fg; const int32_t* target_gt_idx; const float* target_score;
  const float* target_scores_sum;
  const float* grad_scale;
  float batch_scale;
  ydbl_view gbox[3], gcls[3];
} ydbl_loss_grad_desc;
int ydbl_detect_loss_grad(const ydbl_loss_grad_desc* d, void* stream);

/* ConvTranspose2d(cin, cout, kernel 2, stride 2, pad 0) + bias + activation on NHWC views, one launch:
 *   y[n][2i+dy][2j+dx][co] = act(bias[co] + sum_ci x[n][i][j][ci] * W[ci][co][dy][dx]).
 * A GEMM with M = n*h*w, N = 4*cout, K = cin on MFMA (f16: 16x16x32, f32: exact 16x16x4, fp32 accumulation) whose four
 * N-quarters are stored to the four (dy, dx) output pixels straight from the accumulators.
 * x: [n,h,w,cin], y: [n,2h,2w,cout], the same dtype, 16-byte aligned channel vectors, any channel stride (lanes
 * between c and cs are not touched); y must not overlap x.  cin and cout multiples of 32, else YDBL_EINVAL.
 * w: packed on the host, [2*dy+dx][cout][cin] in the view dtype (torch's [cin][cout][2][2] permuted (2, 3, 1, 0)),
 * 16-byte aligned.  bias: fp32 [cout], 16-byte aligned, or NULL.  act: a YDBL_ACT_* code. */
typedef struct {
  ydbl_view x, y;
  const void* w;
  const float* bias;
  int32_t act;
} ydbl_deconv_desc;
int ydbl_deconv2x2_nhwc(const ydbl_deconv_desc* d, void* stream);

/* Instance masks (process_mask / process_mask_native, U/utils/ops.py:644-737), one launch for a batch.
 * For image b and slot k < min(count[b], max_det), with coefficients c (below) and the box
 * (x1, y1, x2, y2) = (det[0] * sx, det[1] * sy, det[2] * sx, det[3] * sy) of row k (fp32 products):
 *   m[r][q] = sum_j c[j] * float(proto[b][r][q][j])        fp32, over the proto grid
 *   crop_after = 0: m is zeroed where not (q >= x1 && q < x2 && r >= y1 && r < y2) (float compares on the proto grid's
 *     own indices), the window rows top..bottom-1, columns left..right-1 of it are resampled to (out_h, out_w)
 *     bilinearly (torch's upsample_bilinear2d, align_corners=False: scale = float(in) / out,
 *     src = max(scale * (d + 0.5) - 0.5, 0), i0 = int(src), i1 = min(i0 + 1, in - 1)), and the output is v > 0
 *     -- process_mask with sx = fp32(mw / iw), sy = fp32(mh / ih) and the whole grid as the window; out_h, out_w equal
 *     to the window is upsample=False (the resampling is then the identity);
 *   crop_after = 1: the window is resampled first, the indicator is applied on the OUTPUT grid's indices, then > 0
 *     -- process_mask_native with sx = sy = 1 and scale_masks' window.
 * The plane of (b, k) is out + (row_offset[b] + k) * out_h * out_w elements, fp32 0 / 1 (YDBL_MASK_F32, the
 * reference's) or uint8 0 / 1 (YDBL_MASK_U8); slots at or past the count write nothing.
 * YDBL_MASK_BITS: the same values as bit planes, out_h * ceil(out_w / 64) uint64 words per plane, (b, k) at
 * out + (row_offset[b] + k) * out_h * ceil(out_w / 64) words; bit j of word q of a row is pixel 64 q + j, bits past
 * out_w are 0; out 8-byte aligned.  1/32 of the fp32 bytes: what ydbl_mask_iou reads.
 * Coefficients: coef != NULL: fp32 [n][max_det][nm] given directly (mc, keep_idx unused).  Otherwise keep_idx
 * int32 [n][max_det] (ydbl_nms's out_idx) names the anchor -- keep_idx itself when nc == 0, keep_idx / nc for the
 * multi-label index anchor * nc + cls -- and the coefficients are that anchor's nm values of the level maps
 * mc[0..nl) ([n,h_l,w_l,nm] views, f16 or f32, anchors counted level after level, row-major); an index outside the
 * levels gives zero coefficients (an all-zero mask).
 * proto: [n,mh,mw,nm] view, f16 or f32, 16-byte aligned channel vectors; nm a multiple of 8, <= 64.
 * det: fp32 rows of det_row floats (0 = 6) whose first four are the box, det_stride floats between images
 * (0 = max_det * det_row).  row_offset: int64 [n] on the device.  1 <= max_det <= 4096.  slots: the slot extent of
 * the grid, 0 = max_det; a caller that knows max(count) passes it to launch no idle workgroups (slots past it are
 * not written).  No atomics, every element of a live slot written once: bit-identical from run to run.  One launch
 * on `stream`, no allocation, no sync. */
enum { YDBL_MASK_F32 = 0, YDBL_MASK_U8 = 1, YDBL_MASK_BITS = 2 };
typedef struct {
  ydbl_view proto;
  ydbl_view mc[3];
  int32_t nl, nc;
  const int32_t* keep_idx;
  const float* det;
  int64_t det_stride;
  int32_t det_row, max_det;
  const int32_t* count;
  const float* coef;
  const int64_t* row_offset;
  void* out;
  int32_t out_h, out_w, out_dtype;
  int32_t top, left, bottom, right;
  float sx, sy;
  int32_t crop_after;
  int32_t slots;
} ydbl_mask_desc;
int ydbl_process_mask(const ydbl_mask_desc* d, void* stream);

/* Ground-truth masks of a batch as bit planes in the layout of YDBL_MASK_BITS, and their areas: the first half of
 * SegmentationValidator._process_batch(masks=True) (models/yolo/segment/val.py:204-212).  Labels are grouped by image
 * as in ydbl_match_desc (gt_ofs int32 [n+1]); label g = gt_ofs[b] + l is image b's l-th label.
 *   overlap != 0: src is the index map uint8 [n][gh][gw]; label g's indicator is src[b] == l + 1 (the reference's
 *     torch.where(gt_masks == index, 1.0, 0.0), val.py:206-209); at most 255 labels of an image can be named;
 *   overlap == 0: src is uint8 planes [n_gt][gh][gw] in grouped label order, nonzero = set.
 * (gh, gw) == (out_h, out_w): the indicator is copied.  Otherwise it is resampled bilinearly to (out_h, out_w) and
 * compared with > 0.5 (val.py:210-212: F.interpolate(mode="bilinear", align_corners=False).gt_(0.5)) by the rule of
 * ydbl_process_mask: scale = float(in) / out, src = max(scale * (d + 0.5) - 0.5, 0), i0 = int(src),
 * i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1, v = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11),
 * every operation rounded to fp32 on its own.  At an exact ratio of 4 (mask_ratio, the reference's default) every v
 * is a dyadic fraction that fp32 holds exactly and none equals 0.5, so the bits are torch's.  At other ratios
 * torch's own value can differ from this formula in the last bit and exact 0.5 occurs: the result equals torch's
 * wherever the reference value is not within rounding of 0.5.
 * bits uint64 [n_gt][out_h][ceil(out_w / 64)] (8-byte aligned; bit j of word q of a row = pixel 64 q + j, bits past
 * out_w zero), area int32 [n_gt] = the set pixels of each plane.  Each word is one wavefront ballot; no atomics,
 * every output written once.  One launch on `stream`, no allocation, no sync. */
typedef struct {
  const uint8_t* src;
  int32_t n, gh, gw;
  int32_t overlap;
  const int32_t* gt_ofs;
  int32_t n_gt;
  int32_t out_h, out_w;
  uint64_t* bits;
  int32_t* area;
} ydbl_gt_bits_desc;
int ydbl_gt_mask_bits(const ydbl_gt_bits_desc* d, void* stream);

/* Mask IoU of every label against every detection slot of its own image, on bit planes: mask_iou
 * (utils/metrics.py:137-153) as SegmentationValidator._process_batch calls it (models/yolo/segment/val.py:213).
 * det_bits: the YDBL_MASK_BITS planes of ydbl_process_mask, (b, k) at (row_offset[b] + k) * out_h * ceil(out_w / 64)
 * words, k < min(count[b], max_det); gt_bits / area_gt: ydbl_gt_mask_bits' outputs, gt_ofs as there.
 *   inter(g, k) = popcount(gt[g] & det[b][k]),  area_det(b, k) = popcount(det[b][k]),
 *   iou = float(inter) / (((float(area_gt) + float(area_det)) - float(inter)) + 1e-7f)      (fp32, no contraction).
 * out_h * out_w <= 2^24 (else YDBL_EINVAL): the counts are then exact in fp32, so iou is bitwise what the
 * reference's fp32 matmul / sum / division gives on 0 / 1 masks.
 * iou fp32 [n_gt][max_det]; inter int32 [n_gt][max_det] and area_det int32 [n][max_det] are optional (NULL skips);
 * columns / slots at or past the count are written 0.  No atomics, every output element written exactly once:
 * identical from run to run.  One launch on `stream`, no allocation, no sync. */
typedef struct {
  const uint64_t* det_bits;
  const int64_t* row_offset;
  const int32_t* count;
  int32_t n, max_det;
  const uint64_t* gt_bits;
  const int32_t* gt_ofs;
  const int32_t* area_gt;
  int32_t n_gt;
  int32_t out_h, out_w;
  float* iou;
  int32_t* inter;
  int32_t* area_det;
} ydbl_mask_iou_desc;
int ydbl_mask_iou(const ydbl_mask_iou_desc* d, void* stream);

/* ydbl_match_predictions with the IoU of a pair read from a matrix instead of computed from boxes: the second half of
 * SegmentationValidator._process_batch(masks=True) (models/yolo/segment/val.py:217, BaseValidator.match_predictions
 * engine/validator.py:222-262).  iou fp32 [n_gt][max_det] as ydbl_mask_iou writes it (row g: label g against the
 * slots of its own image); det supplies the class column only.  Everything else -- class mismatch = IoU 0,
 * single_cls, correct uint8 [n][max_det][n_iou], rows >= det_count zeroed, the workspace of ydbl_match_workspace,
 * the larger label index on an exact tie -- is ydbl_match_predictions' rule, the same kernel. */
typedef struct {
  const float* det; const int32_t* det_count;
  int32_t n, max_det;
  const float* iou;
  const float* gt_cls; const int32_t* gt_ofs;
  int32_t n_gt;
  const float* iouv; int32_t n_iou;
  int32_t single_cls;
  uint8_t* correct;
  void* workspace; /* ydbl_match_workspace(n, max_det, n_gt, n_iou) bytes */
} ydbl_match_iou_desc;
int ydbl_match_iou(const ydbl_match_iou_desc* d, void* stream);

/* Keypoints of the kept detections of a pose model (Pose.kpts_decode, nn/modules/head.py:396-401), one launch for a
 * batch, behind ydbl_nms in the same graph.  For image b and slot k < min(count[b], max_det), keep_idx int32
 * [n][max_det] (ydbl_nms's out_idx) names the anchor -- keep_idx itself when nc == 0, keep_idx / nc for the
 * multi-label index anchor * nc + cls, ydbl_process_mask's rule -- and the anchor's K * ndim raw values are read from
 * the level maps kpt[0..nl) ([n,h_l,w_l,K*ndim] views, f16 or f32, any channel stride >= K * ndim, anchors counted
 * level after level, row-major).  With (gx, gy) the anchor's grid cell and s = stride[l] of its level, in fp32 from the
 * stored value, every operation rounded on its own:
 *   x = (v_x * 2 + gx) * s,   y = (v_y * 2 + gy) * s,   visibility = 1 / (1 + expf(-v))   (ndim == 3 only).
 * v * 2 and * s are exact for the power-of-two strides, so x / y equal torch's fp32 evaluation of the reference formula
 * on the same stored values bit for bit.  (Under half=True the reference decodes in fp16; this does not.)
 * out fp32 [n][max_det][K][ndim], letterboxed-input pixels.  Slots at or past the count are written 0; an index outside
 * the levels (or negative) gives a zero row.  No atomics, every output element written exactly once: identical from
 * run to run.  1 <= max_det <= 4096, ndim 2 or 3.  One launch on `stream`, no allocation, no sync. */
typedef struct {
  ydbl_view kpt[3];
  int32_t nl, nc;
  float stride[3];
  const int32_t* keep_idx;
  const int32_t* count;
  int32_t n, max_det;
  int32_t K, ndim;
  float* out;
} ydbl_pose_kpt_desc;
int ydbl_pose_keypoints(const ydbl_pose_kpt_desc* d, void* stream);

/* Object keypoint similarity of every label against every detection slot of its own image: kpt_iou
 * (utils/metrics.py:156-175) as PoseValidator._process_batch calls it (models/yolo/pose/val.py:190-193).  Labels are
 * grouped by image as in ydbl_match_desc (gt_ofs int32 [n+1]); label g = gt_ofs[b] + l is image b's l-th label.
 * pred_kpts fp32 [n][max_det][K][ndim] (ydbl_pose_keypoints' layout; only x, y are read), gt_kpts fp32 [n_gt][K][3]
 * (x, y, visibility), gt_box fp32 [n_gt][4] xyxy, sigma fp32 [K].  In fp32, no contraction:
 *   area = ((x2 - x1) * (y2 - y1)) * 0.53f,
 *   e_k  = ((gx - px)^2 + (gy - py)^2) / ((((2 sigma_k)^2) * (area + 1e-7f)) * 2),
 *   oks  = (sum of expf(-e_k) over the label's points with visibility != 0, in keypoint order) / (n_visible + 1e-7f).
 * A label with no visible point gives 0.  oks fp32 [n_gt][max_det], ydbl_mask_iou's layout: row g against the slots
 * of its own image, columns at or past the count written 0 -- what ydbl_match_iou reads.  K <= 64.  No atomics,
 * every output element written exactly once.  One launch on `stream`, no allocation, no sync. */
typedef struct {
  const float* pred_kpts;
  const int32_t* count;
  int32_t n, max_det;
  int32_t K, ndim;
  const float* gt_kpts;
  const float* gt_box;
  const int32_t* gt_ofs;
  int32_t n_gt;
  const float* sigma;
  float* oks;
} ydbl_kpt_oks_desc;
int ydbl_kpt_oks(const ydbl_kpt_oks_desc* d, void* stream);

const char* ydbl_last_error(void);
const char* ydbl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* YDBL_H */
