// Pose models, gfx950: the kept detections' keypoints (Pose.kpts_decode, U/nn/modules/head.py:396-401) behind the NMS,
// and the OKS matrix of validation (kpt_iou, U/utils/metrics.py:156-175, as PoseValidator._process_batch calls it,
// U/models/yolo/pose/val.py:190-193).
//
// pose_keypoints_kernel: one thread per (image, detection slot, keypoint).  The slot's keep_idx (ydbl_nms's out_idx)
// names the anchor by ydbl_process_mask's rule -- keep_idx itself when nc == 0, keep_idx / nc for the multi-label
// index -- the anchor names a level and a grid cell (gx, gy), and the keypoint's ndim raw values are read from the
// level's map and decoded in fp32:
//   x = (v_x * 2 + gx) * stride,  y = (v_y * 2 + gy) * stride,  visibility = 1 / (1 + expf(-v))  (ndim == 3).
// v * 2 and * stride are exact (the strides are powers of two), so x / y carry the one rounding of the addition:
// torch's fp32 evaluation of the reference formula on the same stored values, bit for bit.  A slot at or past
// count[image], or an index outside the levels, is written 0.  Every output element has one writer.
//
// kpt_oks_kernel: grid (ceil(max_det / 64), images), four waves per workgroup.  Lane j of every wave owns detection
// slot 64 * blockIdx.x + j; wave w takes the image's labels l = w (mod 4).  The label's keypoints, area and the
// sigmas are wave-uniform loads, the slot's keypoints per-lane ones; the K <= 64 terms are summed in keypoint order,
// each operation rounded to fp32 on its own.  No LDS, no atomics, every output element written exactly once.
#include "decode_math.hpp"

#pragma clang fp contract(off)

namespace ydbl {
namespace {

constexpr int PK_THREADS = 256;

struct KptArgs {
  const void* kp[3]; int lh[3], lw[3], lcs[3], ldt[3]; float st[3]; int nl;
  const int* keep_idx; const int* count; int nc;
  int n, max_det, K, ndim;
  float* out;
};

__device__ __forceinline__ float pk_load(const void* p, int dt, int64_t e) {
  return dt == YDBL_F16 ? float(reinterpret_cast<const _Float16*>(p)[e]) : reinterpret_cast<const float*>(p)[e];
}

__global__ __launch_bounds__(PK_THREADS) void pose_keypoints_kernel(KptArgs a) {
  const int64_t i = (int64_t)blockIdx.x * PK_THREADS + threadIdx.x;
  if (i >= (int64_t)a.n * a.max_det * a.K) return;
  const int k = int(i % a.K);
  const int64_t ds = i / a.K;
  const int slot = int(ds % a.max_det), b = int(ds / a.max_det);
  float x = 0.f, y = 0.f, v = 0.f;
  if (slot < min(a.count[b], a.max_det)) {
    int idx = a.keep_idx[ds];
    if (a.nc > 0 && idx >= 0) idx /= a.nc;
    for (int l = 0; l < a.nl && idx >= 0; ++l) {
      const int hw = a.lh[l] * a.lw[l];
      if (idx < hw) {
        const int gy = idx / a.lw[l], gx = idx - gy * a.lw[l];
        const int64_t e = ((int64_t)b * hw + idx) * a.lcs[l] + (int64_t)k * a.ndim;
        x = (pk_load(a.kp[l], a.ldt[l], e) * 2.0f + float(gx)) * a.st[l];
        y = (pk_load(a.kp[l], a.ldt[l], e + 1) * 2.0f + float(gy)) * a.st[l];
        if (a.ndim == 3) v = cls_score(pk_load(a.kp[l], a.ldt[l], e + 2));
        break;
      }
      idx -= hw;  // an index past the last level (or negative) leaves the row zero
    }
  }
  float* o = a.out + i * a.ndim;
  o[0] = x; o[1] = y;
  if (a.ndim == 3) o[2] = v;
}

struct OksArgs {
  const float* pred; int ndim;
  const int* count; int n, max_det;
  const float* gt_kpts; const float* gt_box; const int* gt_ofs; int n_gt;
  const float* sigma; int K;
  float* oks;
};

__global__ __launch_bounds__(PK_THREADS) void kpt_oks_kernel(OksArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = blockIdx.x * 64 + lane;
  if (d >= a.max_det) return;
  const int g0 = min(max(a.gt_ofs[b], 0), a.n_gt);
  const int nl = min(max(a.gt_ofs[b + 1], g0), a.n_gt) - g0;
  const bool live = d < min(a.count[b], a.max_det);
  const float* pk = a.pred + ((int64_t)b * a.max_det + d) * a.K * a.ndim;
  for (int l = wave; l < nl; l += PK_THREADS / 64) {
    const int g = g0 + l;
    float r = 0.f;
    if (live) {
      const float* gk = a.gt_kpts + (int64_t)g * a.K * 3;
      const float* gb = a.gt_box + (int64_t)g * 4;
      const float area = ((gb[2] - gb[0]) * (gb[3] - gb[1])) * 0.53f;  // xyxy2xywh(bbox)[:, 2:].prod(1) * 0.53
      const float ae = area + 1e-7f;
      float sum = 0.f, nv = 0.f;
      for (int k = 0; k < a.K; ++k) {
        if (gk[3 * k + 2] == 0.f) continue;  // kpt_mask: an invisible label point adds exactly 0
        const float dx = gk[3 * k] - pk[k * a.ndim], dy = gk[3 * k + 1] - pk[k * a.ndim + 1];
        const float dd = dx * dx + dy * dy;
        const float s2 = 2.0f * a.sigma[k];
        const float e = dd / (((s2 * s2) * ae) * 2.0f);
        sum += expf(-e);
        nv += 1.f;
      }
      r = sum / (nv + 1e-7f);
    }
    a.oks[(int64_t)g * a.max_det + d] = r;
  }
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_pose_keypoints(const ydbl_pose_kpt_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "pose_keypoints: null descriptor");
  if (!d->keep_idx || !d->count || !d->out) return fail(YDBL_EINVAL, "pose_keypoints: null buffer");
  if (d->nl < 1 || d->nl > 3) return fail(YDBL_EINVAL, "pose_keypoints: nl must be in [1, 3]");
  if (d->nc < 0) return fail(YDBL_EINVAL, "pose_keypoints: nc must be >= 0");
  if (d->n < 1 || d->max_det < 1 || d->max_det > 4096)
    return fail(YDBL_EINVAL, "pose_keypoints: n >= 1 and max_det in [1, 4096] expected");
  if (d->K < 1 || (d->ndim != 2 && d->ndim != 3)) return fail(YDBL_EINVAL, "pose_keypoints: K >= 1, ndim 2 or 3");
  KptArgs a{};
  for (int l = 0; l < d->nl; ++l) {
    if (int rc = check_view(&d->kpt[l], "pose_keypoints kpt", false)) return rc;
    if (d->kpt[l].c != d->K * d->ndim || d->kpt[l].n != d->n)
      return fail(YDBL_EINVAL, "pose_keypoints: kpt levels must be [n, h, w, K * ndim]");
    if ((int64_t)d->kpt[l].h * d->kpt[l].w >= (int64_t)1 << 30) return fail(YDBL_EINVAL, "pose_keypoints: level too large");
    a.kp[l] = d->kpt[l].ptr; a.lh[l] = d->kpt[l].h; a.lw[l] = d->kpt[l].w; a.lcs[l] = d->kpt[l].cs;
    a.ldt[l] = d->kpt[l].dtype; a.st[l] = d->stride[l];
  }
  a.nl = d->nl; a.keep_idx = d->keep_idx; a.count = d->count; a.nc = d->nc;
  a.n = d->n; a.max_det = d->max_det; a.K = d->K; a.ndim = d->ndim; a.out = d->out;
  const int64_t total = (int64_t)d->n * d->max_det * d->K;
  const int64_t blocks = cdiv(total, PK_THREADS);
  if (blocks >= (int64_t)1 << 31) return fail(YDBL_EINVAL, "pose_keypoints: output too large");
  pose_keypoints_kernel<<<(unsigned)blocks, PK_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch("ydbl_pose_keypoints");
}

extern "C" int ydbl_kpt_oks(const ydbl_kpt_oks_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "kpt_oks: null descriptor");
  if (!d->pred_kpts || !d->count || !d->gt_ofs || !d->sigma) return fail(YDBL_EINVAL, "kpt_oks: null buffer");
  if (d->n < 1 || d->n > 65535 || d->max_det < 1) return fail(YDBL_EINVAL, "kpt_oks: n must be in [1, 65535], max_det >= 1");
  if (d->K < 1 || d->K > 64 || (d->ndim != 2 && d->ndim != 3))
    return fail(YDBL_EINVAL, "kpt_oks: K must be in [1, 64], ndim 2 or 3");
  if (d->n_gt < 0 || (d->n_gt > 0 && (!d->gt_kpts || !d->gt_box || !d->oks)))
    return fail(YDBL_EINVAL, "kpt_oks: null buffer (labels missing)");
  if (d->n_gt == 0) return YDBL_OK;
  OksArgs a;
  a.pred = d->pred_kpts; a.ndim = d->ndim; a.count = d->count; a.n = d->n; a.max_det = d->max_det;
  a.gt_kpts = d->gt_kpts; a.gt_box = d->gt_box; a.gt_ofs = d->gt_ofs; a.n_gt = d->n_gt;
  a.sigma = d->sigma; a.K = d->K; a.oks = d->oks;
  const dim3 grid((unsigned)cdiv(d->max_det, 64), (unsigned)d->n);
  kpt_oks_kernel<<<grid, PK_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch("ydbl_kpt_oks");
}
