// Validation-side matching of NMS detections to ground-truth labels on the device: the mAP TP matrix
// (match_kernel) and, further down, the confusion matrix (confusion_kernel) on the same tensors.
//
// Restates DetectionValidator._process_batch (U/models/yolo/detect/val.py:209-227) =
// box_iou (U/utils/metrics.py:52-71) + BaseValidator.match_predictions non-scipy branch
// (U/engine/validator.py:222-262).  That routine, per IoU threshold t, takes every
// (label, detection) pair with class-masked IoU >= t, sorts them by IoU descending, keeps the
// first pair per detection (its highest-IoU label) and then, in detection order, the first pair
// per label.  Hence, for one image:
//   best(d)   = argmax over labels of the class-masked IoU (exact ties -> larger label index, the
//               order numpy's reversed stable argsort gives for small match arrays),
//   correct[d][t] = maxIoU(d) >= t  and  no d' < d with best(d') == best(d) and maxIoU(d') >= t.
// The second condition is a per-(label, threshold) atomicMin of the detection index.
//
// One 256-thread workgroup per image.  IoU is evaluated in fp32 with the reference's operation
// order and no FMA contraction, so it is bitwise the torch CPU value and the threshold compares
// agree exactly.
//
// match_kernel is a template on where the IoU of a pair comes from: pair_iou on the boxes (ydbl_match_predictions),
// or a given matrix iou[label][slot] (ydbl_match_iou: the mask IoUs of ydbl_mask_iou,
// SegmentationValidator._process_batch(masks=True), U/models/yolo/segment/val.py:173-217).  The rule is one.
#include <climits>

#include "common.hpp"

#pragma clang fp contract(off)

namespace ydbl {

constexpr int MATCH_THREADS = 256;
constexpr int MATCH_MAX_IOU = 32;

struct MatchArgs {
  const float* det; const int* det_count;
  int n, max_det;
  const float* gt_box; const float* gt_cls; const int* gt_ofs;
  const float* iou;  // MATRIX: [n_gt][max_det], row g = label g against the slots of its own image
  const float* iouv; int n_iou;
  int single_cls;
  int* min_det;  // [n_gt][n_iou]
  int* best;     // [n][max_det]
  int* valid;    // [n][max_det] bitmask over thresholds
  uint8_t* correct;
};

// box_iou (U/utils/metrics.py:52-71) for one pair, same rounding sequence as the torch CPU op.
__device__ __forceinline__ float pair_iou(const float* a, const float* b) {
  const float iw = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.0f);
  const float ih = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.0f);
  const float inter = iw * ih;
  const float area_a = (a[2] - a[0]) * (a[3] - a[1]);
  const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / (((area_a + area_b) - inter) + 1e-7f);
}

template <bool MATRIX>
__global__ __launch_bounds__(MATCH_THREADS) void match_kernel(MatchArgs p) {
  const int b = blockIdx.x;
  const int g0 = p.gt_ofs[b], nl = p.gt_ofs[b + 1] - g0;
  const int nd = min(p.det_count[b], p.max_det);
  const float* det = p.det + (int64_t)b * p.max_det * 6;
  uint8_t* out = p.correct + (int64_t)b * p.max_det * p.n_iou;

  for (int i = threadIdx.x; i < nl * p.n_iou; i += MATCH_THREADS)
    __hip_atomic_store(p.min_det + (int64_t)g0 * p.n_iou + i, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  __syncthreads();

  for (int d = threadIdx.x; d < nd; d += MATCH_THREADS) {
    const float* db = det + d * 6;
    const float dc = p.single_cls ? 0.0f : db[5];
    int best = -1;
    float bi = 0.0f;
    for (int l = 0; l < nl; ++l) {
      // iou * (true_cls == pred_cls): a class mismatch contributes an IoU of exactly 0
      float v = 0.0f;
      if (p.gt_cls[g0 + l] == dc) {
        if constexpr (MATRIX) v = p.iou[(int64_t)(g0 + l) * p.max_det + d];
        else v = pair_iou(p.gt_box + (int64_t)(g0 + l) * 4, db);
      }
      if (best < 0 || v >= bi) { bi = v; best = l; }
    }
    int mask = 0;
    if (best >= 0)
      for (int t = 0; t < p.n_iou; ++t)
        if (bi >= p.iouv[t]) {
          mask |= 1 << t;
          atomicMin(p.min_det + (int64_t)(g0 + best) * p.n_iou + t, d);
        }
    p.best[(int64_t)b * p.max_det + d] = best;
    p.valid[(int64_t)b * p.max_det + d] = mask;
  }
  __threadfence();
  __syncthreads();

  for (int d = threadIdx.x; d < p.max_det; d += MATCH_THREADS) {
    const int best = d < nd ? p.best[(int64_t)b * p.max_det + d] : -1;
    const int mask = d < nd ? p.valid[(int64_t)b * p.max_det + d] : 0;
    for (int t = 0; t < p.n_iou; ++t) {
      bool ok = false;
      if ((mask >> t) & 1)
        ok = __hip_atomic_load(p.min_det + (int64_t)(g0 + best) * p.n_iou + t, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT) == d;
      out[d * p.n_iou + t] = ok;
    }
  }
}

// ---- confusion matrix ---------------------------------------------------------------------------
// Restates ConfusionMatrix.process_batch (U/utils/metrics.py:326-382) for a batch of images, one workgroup per
// image.  The reference takes every (label, detection) pair with iou > iou_thres, sorts by IoU descending and
// keeps the first pair per detection (np.unique on column 1), sorts again and keeps the first pair per label
// (np.unique on column 0).  That is two maximum selections:
//   best(d)   = argmax over labels of the participating IoU of detection d,
//   winner(l) = argmax over detections with best(d) == l of iou(l, d),
// both taken here as an atomic max over a packed 64-bit key, iou bits << 32 | index.  A participating IoU is a
// positive float (iou > iou_thres >= 0), so its bit pattern orders as an unsigned integer and a key is never 0;
// the index in the low word makes the tie rule ours: on bit-equal IoU the larger label index wins best(d) and
// the larger detection index wins winner(l), which is what numpy's reversed argsort gives for match arrays of
// up to 16 rows (its order on ties is unspecified above that).
// The pair work is spread over the workgroup: a chunk of labels is staged in LDS, the threads form a
// (256 / lw) x lw grid with lw = the chunk length rounded up to a power of two, a thread keeps its label and
// walks the detections in steps of 256 / lw.  Per-detection keys live in LDS while max_det <= CM_DET_LDS,
// otherwise in the workspace; per-label keys in the workspace.  The (nc+1)^2 counts are privatised in LDS while
// they fit CM_LDS_CELLS (nc <= 80, 26 KB) and flushed with one atomic add per non-zero cell; above that they
// go straight to the global matrix.  All sums are integer, so the result does not depend on scheduling.
constexpr int CM_THREADS = 256;
constexpr int CM_CHUNK = 256;           // labels staged per pass (4 KB)
constexpr int CM_DET_LDS = 1024;        // per-detection keys in LDS up to this max_det (8 KB)
constexpr int CM_LDS_CELLS = 81 * 81;   // privatised counts up to nc = 80 (26 KB)
constexpr int CM_MAX_NC = 32767;
constexpr int CM_MAX_DET = 1 << 20;

using u64 = unsigned long long;

struct ConfusionArgs {
  const float* det; const int* det_count;
  int n, max_det;
  const float* gt_box; const float* gt_cls; const int* gt_ofs;
  int n_gt, nc;
  float conf, iou_thres;
  u64* matrix;  // [(nc+1)][(nc+1)]
  int* invalid;
  u64* lkey;    // [n_gt]
  u64* dkey;    // [n][max_det], used when max_det > CM_DET_LDS
};

// the reference's .int() of a class, or -1 outside [0, nc) (where the reference's matrix index raises)
__device__ __forceinline__ int cls_index(float c, int nc) { return c > -1.0f && c < (float)nc ? (int)c : -1; }

template <bool DET_LDS, bool CNT_LDS>
__global__ __launch_bounds__(CM_THREADS) void confusion_kernel(ConfusionArgs p) {
  __shared__ u64 s_dkey[DET_LDS ? CM_DET_LDS : 1];
  __shared__ float s_box[CM_CHUNK * 4];
  __shared__ int s_cnt[CNT_LDS ? CM_LDS_CELLS : 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int g0 = min(max(p.gt_ofs[b], 0), p.n_gt);
  const int nl = min(max(p.gt_ofs[b + 1], g0), p.n_gt) - g0;
  const int nd = max(min(p.det_count[b], p.max_det), 0);
  const float* det = p.det + (int64_t)b * p.max_det * 6;
  u64* dkey = DET_LDS ? s_dkey : p.dkey + (int64_t)b * p.max_det;
  u64* lkey = p.lkey + g0;
  const int side = p.nc + 1, cells = side * side;

  auto load_dkey = [&](int d) -> u64 {
    if constexpr (DET_LDS) return dkey[d];
    else return __hip_atomic_load(dkey + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto count = [&](int row, int col) {
    if (row < 0 || col < 0) atomicAdd(p.invalid, 1);
    else if constexpr (CNT_LDS) atomicAdd(&s_cnt[row * side + col], 1);
    else atomicAdd(p.matrix + (int64_t)row * side + col, (u64)1);
  };

  for (int d = tid; d < nd; d += CM_THREADS) {
    if constexpr (DET_LDS) dkey[d] = 0;
    else __hip_atomic_store(dkey + d, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int l = tid; l < nl; l += CM_THREADS)
    __hip_atomic_store(lkey + l, (u64)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if constexpr (CNT_LDS)
    for (int i = tid; i < cells; i += CM_THREADS) s_cnt[i] = 0;
  __threadfence();

  // best(d): every participating pair, one chunk of labels at a time
  for (int c0 = 0; c0 < nl; c0 += CM_CHUNK) {
    const int cl = min(CM_CHUNK, nl - c0);
    __syncthreads();  // the keys are zeroed / the previous chunk is consumed
    for (int i = tid; i < cl * 4; i += CM_THREADS) s_box[i] = p.gt_box[(int64_t)(g0 + c0) * 4 + i];
    __syncthreads();
    int lw_log = 0;
    while ((1 << lw_log) < cl) ++lw_log;
    const int l = tid & ((1 << lw_log) - 1), d0 = tid >> lw_log, dstep = CM_THREADS >> lw_log;
    if (l < cl) {
      const float lb[4] = {s_box[l * 4], s_box[l * 4 + 1], s_box[l * 4 + 2], s_box[l * 4 + 3]};
      for (int d = d0; d < nd; d += dstep) {
        const float* db = det + d * 6;
        if (!(db[4] > p.conf)) continue;
        const float v = pair_iou(lb, db);
        if (v > p.iou_thres) atomicMax(dkey + d, ((u64)__float_as_uint(v) << 32) | (unsigned)(c0 + l));
      }
    }
  }
  __threadfence();
  __syncthreads();

  // winner(l): each detection with a best label bids for it with its IoU
  for (int d = tid; d < nd; d += CM_THREADS) {
    const u64 k = load_dkey(d);
    if (k) atomicMax(lkey + (unsigned)k, (k & 0xffffffff00000000ull) | (unsigned)d);
  }
  __threadfence();
  __syncthreads();

  for (int l = tid; l < nl; l += CM_THREADS) {
    const u64 k = __hip_atomic_load(lkey + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int col = cls_index(p.gt_cls[g0 + l], p.nc);
    count(k ? cls_index(det[(int64_t)(unsigned)k * 6 + 5], p.nc) : p.nc, col);  // matched / missed (background row)
  }
  for (int d = tid; d < nd; d += CM_THREADS) {
    if (!(det[d * 6 + 4] > p.conf)) continue;
    const u64 k = load_dkey(d);
    const bool won = k && (unsigned)__hip_atomic_load(lkey + (unsigned)k, __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT) == (unsigned)d;
    if (!won) count(cls_index(det[d * 6 + 5], p.nc), p.nc);  // predicted background
  }
  if constexpr (CNT_LDS) {
    __syncthreads();
    for (int i = tid; i < cells; i += CM_THREADS)
      if (s_cnt[i]) atomicAdd(p.matrix + i, (u64)s_cnt[i]);
  }
}

}  // namespace ydbl

using namespace ydbl;

extern "C" int64_t ydbl_match_workspace(int32_t n, int32_t max_det, int32_t n_gt, int32_t n_iou) {
  if (n < 0 || max_det < 0 || n_gt < 0 || n_iou < 0) return -1;
  return 4 * ((int64_t)n_gt * n_iou + 2 * (int64_t)n * max_det) + 16;
}

extern "C" int ydbl_match_predictions(const ydbl_match_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "match: null descriptor");
  if (!d->det || !d->det_count || !d->gt_ofs || !d->iouv || !d->correct || !d->workspace)
    return fail(YDBL_EINVAL, "match: null buffer");
  if (d->n < 1 || d->max_det < 1) return fail(YDBL_EINVAL, "match: empty batch");
  if (d->n_gt < 0 || (d->n_gt > 0 && (!d->gt_box || !d->gt_cls)))
    return fail(YDBL_EINVAL, "match: labels missing");
  if (d->n_iou < 1 || d->n_iou > MATCH_MAX_IOU) return fail(YDBL_EINVAL, "match: n_iou must be in [1, 32]");
  MatchArgs a;
  a.det = d->det; a.det_count = d->det_count; a.n = d->n; a.max_det = d->max_det;
  a.gt_box = d->gt_box; a.gt_cls = d->gt_cls; a.gt_ofs = d->gt_ofs; a.iou = nullptr;
  a.iouv = d->iouv; a.n_iou = d->n_iou; a.single_cls = d->single_cls;
  a.min_det = reinterpret_cast<int*>(d->workspace);
  a.best = a.min_det + (int64_t)d->n_gt * d->n_iou;
  a.valid = a.best + (int64_t)d->n * d->max_det;
  a.correct = d->correct;
  match_kernel<false><<<d->n, MATCH_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch("ydbl_match_predictions");
}

extern "C" int ydbl_match_iou(const ydbl_match_iou_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "match_iou: null descriptor");
  if (!d->det || !d->det_count || !d->gt_ofs || !d->iouv || !d->correct || !d->workspace)
    return fail(YDBL_EINVAL, "match_iou: null buffer");
  if (d->n < 1 || d->max_det < 1) return fail(YDBL_EINVAL, "match_iou: empty batch");
  if (d->n_gt < 0 || (d->n_gt > 0 && (!d->iou || !d->gt_cls)))
    return fail(YDBL_EINVAL, "match_iou: labels or IoU matrix missing");
  if (d->n_iou < 1 || d->n_iou > MATCH_MAX_IOU) return fail(YDBL_EINVAL, "match_iou: n_iou must be in [1, 32]");
  MatchArgs a;
  a.det = d->det; a.det_count = d->det_count; a.n = d->n; a.max_det = d->max_det;
  a.gt_box = nullptr; a.gt_cls = d->gt_cls; a.gt_ofs = d->gt_ofs; a.iou = d->iou;
  a.iouv = d->iouv; a.n_iou = d->n_iou; a.single_cls = d->single_cls;
  a.min_det = reinterpret_cast<int*>(d->workspace);
  a.best = a.min_det + (int64_t)d->n_gt * d->n_iou;
  a.valid = a.best + (int64_t)d->n * d->max_det;
  a.correct = d->correct;
  match_kernel<true><<<d->n, MATCH_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch("ydbl_match_iou");
}

extern "C" int64_t ydbl_confusion_workspace(int32_t n, int32_t max_det, int32_t n_gt) {
  if (n < 0 || max_det < 0 || n_gt < 0) return -1;
  return 8 * ((int64_t)n_gt + (max_det > CM_DET_LDS ? (int64_t)n * max_det : 0)) + 16;
}

extern "C" int ydbl_confusion_matrix(const ydbl_confusion_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "confusion: null descriptor");
  if (!d->det || !d->det_count || !d->gt_ofs || !d->matrix || !d->invalid || !d->workspace)
    return fail(YDBL_EINVAL, "confusion: null buffer");
  if (d->n < 1 || d->max_det < 1) return fail(YDBL_EINVAL, "confusion: empty batch");
  if (d->max_det > CM_MAX_DET) return fail(YDBL_EINVAL, "confusion: max_det must be <= 2^20");
  if (d->n_gt < 0 || (d->n_gt > 0 && (!d->gt_box || !d->gt_cls)))
    return fail(YDBL_EINVAL, "confusion: labels missing");
  if (d->nc < 1 || d->nc > CM_MAX_NC) return fail(YDBL_EINVAL, "confusion: nc must be in [1, 32767]");
  if (!(d->iou_thres >= 0.0f)) return fail(YDBL_EINVAL, "confusion: iou_thres must be >= 0");
  if (reinterpret_cast<uintptr_t>(d->workspace) % 8 || reinterpret_cast<uintptr_t>(d->matrix) % 8)
    return fail(YDBL_EINVAL, "confusion: workspace and matrix must be 8-byte aligned");
  ConfusionArgs a;
  a.det = d->det; a.det_count = d->det_count; a.n = d->n; a.max_det = d->max_det;
  a.gt_box = d->gt_box; a.gt_cls = d->gt_cls; a.gt_ofs = d->gt_ofs; a.n_gt = d->n_gt; a.nc = d->nc;
  a.conf = d->conf; a.iou_thres = d->iou_thres;
  a.matrix = reinterpret_cast<u64*>(d->matrix);
  a.invalid = d->invalid;
  a.lkey = reinterpret_cast<u64*>(d->workspace);
  a.dkey = a.lkey + d->n_gt;
  const bool det_lds = d->max_det <= CM_DET_LDS, cnt_lds = (d->nc + 1) * (d->nc + 1) <= CM_LDS_CELLS;
  hipStream_t s = as_stream(stream);
  if (det_lds && cnt_lds) confusion_kernel<true, true><<<d->n, CM_THREADS, 0, s>>>(a);
  else if (det_lds) confusion_kernel<true, false><<<d->n, CM_THREADS, 0, s>>>(a);
  else if (cnt_lds) confusion_kernel<false, true><<<d->n, CM_THREADS, 0, s>>>(a);
  else confusion_kernel<false, false><<<d->n, CM_THREADS, 0, s>>>(a);
  return check_launch("ydbl_confusion_matrix");
}
