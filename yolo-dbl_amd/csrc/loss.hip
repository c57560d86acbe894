// The detection loss, forward only: v8DetectionLoss.__call__ (U/utils/loss.py:206-260) with bbox_decode (:197-204),
// BboxLoss (:99-113), DFLoss (:73-88), bbox_iou(CIoU=True) (U/utils/metrics.py:74-134) and the TaskAlignedAssigner
// (U/utils/tal.py:40-295, make_anchors :333-345, bbox2dist :360-363), reading the Detect head's NHWC level buffers
// (box logits | class logits) in place.  All arithmetic fp32 whatever the levels' dtype.
//
// Five launches on the caller's stream, nothing allocated, nothing read back:
//   decode   thread per (image, anchor, side): the DFL expectation -> predicted boxes [B][A][4] in grid units; clears
//            the per-anchor pick counters and the per-label maxima.
//   select   one workgroup per (image, label): only the cells whose centre can lie inside the label's box are visited
//            on each level (never all of A).  Each thread keeps the best `topk` (metric, anchor) keys of its cells in
//            registers; the workgroup merges them in topk rounds of a block-wide maximum, then bumps the pick counter
//            of each chosen anchor and leaves its own index there (integer atomics).
//   resolve  thread per (image, anchor): a count of 1 gives the owner; above 1, argmax of the overlaps over ALL the
//            image's labels (first index on ties).  Writes the owner's metric and raises the per-label maxima with
//            atomicMax on the bits of the non-negative floats.
//   terms    thread per (image, anchor): target score, BCE over every class, CIoU and DFL terms for fg anchors; a
//            workgroup's four sums meet in a fixed LDS tree and go to a fixed slot.
//   finish   one workgroup: per image the slots in ascending order, then the images in ascending order; gains and
//            the division by max(sum of target scores, 1).
// No floating-point atomics: every output has the same bits on every run.
// Bytes (B = 4, 640^2, nc = 80, fp16): the levels are read twice by decode / terms (4 x 8400 x 144 x 2 B = 9.7 MB
// each, L2 / Infinity Cache resident behind the head), the workspace is 8 words per anchor (1.1 MB).
#include <math.h>

#include <algorithm>

#include "common.hpp"

namespace ydbl {

constexpr int LS_THREADS = 256;
constexpr int LS_TOPK_MAX = 16;
constexpr int LS_REG = 16;  // reg_max

struct LossLevel {
  const void* box; const void* cls;
  int h, w, bcs, ccs, bf16, cf16;
  int a0;  // first anchor of the level
  float s;
};

struct LossArgs {
  LossLevel lv[3];
  int nl, nc, B, A, M, topk, nblk;
  const float* gt;
  float gain[3];
  // workspace
  float* pbox; int* cnt; int* owner; int* tgt; float* am; unsigned* posm; unsigned* poso; float* part; float* tssimg;
  // outputs
  float* loss; float* tss; float* per_image; int* fg; int* tgi; float* tsc;
};

__device__ __forceinline__ float ld_any(const void* p, int f16, int64_t i) {
  return f16 ? float(reinterpret_cast<const _Float16*>(p)[i]) : reinterpret_cast<const float*>(p)[i];
}

// anchor a of image b -> level, cell; returns the pixel index inside the level's [B][h][w] map
__device__ __forceinline__ int anchor_level(const LossArgs& k, int a, int& gx, int& gy) {
  int l = 0;
  if (k.nl > 1 && a >= k.lv[1].a0) l = 1;
  if (k.nl > 2 && a >= k.lv[2].a0) l = 2;
  const int r = a - k.lv[l].a0;
  gy = r / k.lv[l].w;
  gx = r - gy * k.lv[l].w;
  return l;
}

// bbox_iou(box1, box2, xywh=False, CIoU=True), U/utils/metrics.py:102-130, operation for operation
__device__ __forceinline__ float ciou(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2,
                                      float by2) {
#pragma clang fp contract(off)
  const float eps = 1e-7f;
  const float w1 = ax2 - ax1, h1 = ay2 - ay1 + eps;
  const float w2 = bx2 - bx1, h2 = by2 - by1 + eps;
  const float inter = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.0f) * fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.0f);
  const float uni = w1 * h1 + w2 * h2 - inter + eps;
  const float iou = inter / uni;
  const float cw = fmaxf(ax2, bx2) - fminf(ax1, bx1);
  const float ch = fmaxf(ay2, by2) - fminf(ay1, by1);
  const float c2 = cw * cw + ch * ch + eps;
  const float dx = bx1 + bx2 - ax1 - ax2, dy = by1 + by2 - ay1 - ay2;
  const float rho2 = (dx * dx + dy * dy) / 4.0f;
  const float da = atanf(w2 / h2) - atanf(w1 / h1);
  const float v = 0.4052847345693511f * (da * da);  // 4 / pi^2
  const float alpha = v / (v - iou + 1.0000001f);
  return iou - (rho2 / c2 + v * alpha);
}

struct Gt {
  float cls, x1, y1, x2, y2;
  bool real;
};
__device__ __forceinline__ Gt load_gt(const LossArgs& k, int b, int m) {
#pragma clang fp contract(off)
  const float* g = k.gt + ((int64_t)b * k.M + m) * 5;
  Gt o{g[0], g[1], g[2], g[3], g[4], false};
  o.real = ((o.x1 + o.y1) + (o.x2 + o.y2)) > 0.0f;  // mask_gt: gt_bboxes.sum(2) > 0
  return o;
}
__device__ __forceinline__ int gt_class(const Gt& g, int nc) { return min(max((int)g.cls, 0), nc - 1); }

// select_candidates_in_gts (tal.py:257-262): the anchor centre strictly inside the box
__device__ __forceinline__ bool in_box(const Gt& g, float ax, float ay) {
#pragma clang fp contract(off)
  const float d = fminf(fminf(ax - g.x1, ay - g.y1), fminf(g.x2 - ax, g.y2 - ay));
  return d > 1e-9f;
}

// overlaps and align_metric of (label, anchor) for an anchor inside the label's box (tal.py:132-155)
__device__ __forceinline__ void box_metric(const LossArgs& k, const Gt& g, int b, int a, int l, int gx, int gy,
                                           float& ov, float& metric) {
#pragma clang fp contract(off)
  const float s = k.lv[l].s;
  const f32x4 p = *reinterpret_cast<const f32x4*>(k.pbox + ((int64_t)b * k.A + a) * 4);
  ov = fmaxf(ciou(g.x1, g.y1, g.x2, g.y2, p[0] * s, p[1] * s, p[2] * s, p[3] * s), 0.0f);
  const int64_t pix = ((int64_t)b * k.lv[l].h + gy) * k.lv[l].w + gx;
  const float logit = ld_any(k.lv[l].cls, k.lv[l].cf16, pix * k.lv[l].ccs + gt_class(g, k.nc));
  const float sc = 1.0f / (1.0f + expf(-logit));
  const float o2 = ov * ov;
  metric = sqrtf(sc) * (o2 * o2 * o2);  // alpha 0.5, beta 6
}

__global__ __launch_bounds__(LS_THREADS) void loss_decode_kernel(LossArgs k) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (i < (int64_t)k.B * k.M) {
    k.posm[i] = 0u;
    k.poso[i] = 0u;
  }
  if (i >= (int64_t)k.B * k.A * 4) return;
  const int side = (int)(i & 3);
  const int64_t ba = i >> 2;
  const int b = (int)(ba / k.A), a = (int)(ba - (int64_t)b * k.A);
  if (side == 0) {
    k.cnt[ba] = 0;
    k.owner[ba] = 0x7fffffff;
  }
  int gx, gy;
  const int l = anchor_level(k, a, gx, gy);
  const LossLevel& L = k.lv[l];
  const int64_t base = (((int64_t)b * L.h + gy) * L.w + gx) * L.bcs + side * LS_REG;
  float v[LS_REG];
#pragma unroll
  for (int q = 0; q < LS_REG; ++q) v[q] = ld_any(L.box, L.bf16, base + q);
  float m = v[0];
#pragma unroll
  for (int q = 1; q < LS_REG; ++q) m = fmaxf(m, v[q]);
  float sum = 0.0f, acc = 0.0f;
#pragma unroll
  for (int q = 0; q < LS_REG; ++q) {
    v[q] = expf(v[q] - m);
    sum += v[q];
  }
#pragma unroll
  for (int q = 0; q < LS_REG; ++q) acc += (v[q] / sum) * float(q);  // softmax(3).matmul(proj)
  const float ap = (side & 1 ? float(gy) : float(gx)) + 0.5f;
  k.pbox[i] = side < 2 ? ap - acc : ap + acc;  // dist2bbox(xywh=False)
}

__device__ __forceinline__ void key_insert(uint64_t (&t)[LS_TOPK_MAX], uint64_t key) {
#pragma unroll
  for (int q = 0; q < LS_TOPK_MAX; ++q) {
    const uint64_t hi = key > t[q] ? key : t[q];
    key = key > t[q] ? t[q] : key;
    t[q] = hi;
  }
}

// grid (M, B)
__global__ __launch_bounds__(LS_THREADS) void loss_select_kernel(LossArgs k) {
  __shared__ uint64_t wmax[LS_THREADS / 64];
  __shared__ uint64_t chosen[LS_TOPK_MAX];
  const int m = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const Gt g = load_gt(k, b, m);
  if (!g.real) return;  // (uniform)
  uint64_t best[LS_TOPK_MAX];
#pragma unroll
  for (int q = 0; q < LS_TOPK_MAX; ++q) best[q] = 0;
  for (int l = 0; l < k.nl; ++l) {
    const LossLevel& L = k.lv[l];
    // a rectangle of cells that holds every centre inside the box (one cell of slack; in_box decides)
    const float fw = (float)L.w, fh = (float)L.h;
    const int x0 = (int)fminf(fmaxf(floorf(g.x1 / L.s) - 1.0f, 0.0f), fw);
    const int x1 = (int)fminf(fmaxf(floorf(g.x2 / L.s) + 1.0f, -1.0f), fw - 1.0f);
    const int y0 = (int)fminf(fmaxf(floorf(g.y1 / L.s) - 1.0f, 0.0f), fh);
    const int y1 = (int)fminf(fmaxf(floorf(g.y2 / L.s) + 1.0f, -1.0f), fh - 1.0f);
    const int rw = x1 - x0 + 1, rh = y1 - y0 + 1;
    if (rw <= 0 || rh <= 0 || !(g.x1 == g.x1 && g.x2 == g.x2 && g.y1 == g.y1 && g.y2 == g.y2)) continue;
    for (int c = t; c < rw * rh; c += LS_THREADS) {
      const int gy = y0 + c / rw, gx = x0 + c % rw;
      const float ax = (float(gx) + 0.5f) * L.s, ay = (float(gy) + 0.5f) * L.s;
      if (!in_box(g, ax, ay)) continue;
      const int a = L.a0 + gy * L.w + gx;
      float ov, metric;
      box_metric(k, g, b, a, l, gx, gy, ov, metric);
      // a zero metric counts as not selected (include/ydbl.h); NaN compares false
      if (metric > 0.0f) key_insert(best, ((uint64_t)__float_as_uint(metric) << 32) | (uint32_t)~(uint32_t)a);
    }
  }
  int nsel = 0;
  for (int r = 0; r < k.topk; ++r) {
    uint64_t h = best[0];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)h, d), hi = __shfl_xor((uint32_t)(h >> 32), d);
      const uint64_t o = ((uint64_t)hi << 32) | lo;
      h = o > h ? o : h;
    }
    if ((t & 63) == 0) wmax[t >> 6] = h;
    __syncthreads();
    uint64_t bm = wmax[0];
#pragma unroll
    for (int q = 1; q < LS_THREADS / 64; ++q) bm = wmax[q] > bm ? wmax[q] : bm;
    __syncthreads();
    if (bm == 0) break;  // (uniform) fewer than topk positive metrics
    if (best[0] == bm) {  // anchors are distinct: exactly one thread
#pragma unroll
      for (int q = 0; q + 1 < LS_TOPK_MAX; ++q) best[q] = best[q + 1];
      best[LS_TOPK_MAX - 1] = 0;
      chosen[r] = bm;
    }
    nsel = r + 1;
  }
  __syncthreads();
  if (t < nsel) {
    const int a = (int)~(uint32_t)chosen[t];
    const int64_t ba = (int64_t)b * k.A + a;
    atomicAdd(k.cnt + ba, 1);
    atomicMin(k.owner + ba, m);
  }
}

// grid (nblk, B)
__global__ __launch_bounds__(LS_THREADS) void loss_resolve_kernel(LossArgs k) {
  const int b = blockIdx.y, a = blockIdx.x * LS_THREADS + threadIdx.x;
  if (a >= k.A) return;
  const int64_t ba = (int64_t)b * k.A + a;
  const int c = k.cnt[ba];
  int gx, gy;
  const int l = anchor_level(k, a, gx, gy);
  const float ax = (float(gx) + 0.5f) * k.lv[l].s, ay = (float(gy) + 0.5f) * k.lv[l].s;
  int gi = -1;
  float ov = 0.0f, metric = 0.0f;
  if (c == 1) {
    gi = k.owner[ba];
    box_metric(k, load_gt(k, b, gi), b, a, l, gx, gy, ov, metric);
  } else if (c > 1) {
    // select_highest_overlaps (tal.py:283-295): argmax of overlaps over every label, first index on ties; overlaps
    // are 0 for padding and outside a box
    float bo = -1.0f;
    for (int m = 0; m < k.M; ++m) {
      const Gt g = load_gt(k, b, m);
      float o = 0.0f, mm = 0.0f;
      if (g.real && in_box(g, ax, ay)) box_metric(k, g, b, a, l, gx, gy, o, mm);
      if (o > bo) {
        bo = o; gi = m; ov = o; metric = mm;
      }
    }
  }
  k.tgt[ba] = gi;
  k.am[ba] = metric;
  if (gi >= 0) {
    atomicMax(k.posm + (int64_t)b * k.M + gi, __float_as_uint(fmaxf(metric, 0.0f)));
    atomicMax(k.poso + (int64_t)b * k.M + gi, __float_as_uint(fmaxf(ov, 0.0f)));
  }
  if (k.fg) k.fg[ba] = gi >= 0;
  if (k.tgi) k.tgi[ba] = gi >= 0 ? gi : 0;
}

// grid (nblk, B)
__global__ __launch_bounds__(LS_THREADS) void loss_terms_kernel(LossArgs k) {
#pragma clang fp contract(off)
  __shared__ float red[4][LS_THREADS];
  const int b = blockIdx.y, t = threadIdx.x, a = blockIdx.x * LS_THREADS + t;
  float box = 0.0f, cls = 0.0f, dfl = 0.0f, ts = 0.0f;
  if (a < k.A) {
    const int64_t ba = (int64_t)b * k.A + a;
    int gx, gy;
    const int l = anchor_level(k, a, gx, gy);
    const LossLevel& L = k.lv[l];
    const int64_t pix = ((int64_t)b * L.h + gy) * L.w + gx;
    const int gi = k.tgt[ba];
    int tc = -1;
    Gt g{};
    if (gi >= 0) {
      g = load_gt(k, b, gi);
      tc = gt_class(g, k.nc);
      const float pm = __uint_as_float(k.posm[(int64_t)b * k.M + gi]);
      const float po = __uint_as_float(k.poso[(int64_t)b * k.M + gi]);
      ts = k.am[ba] * po / (pm + 1e-9f);  // tal.py:115
    }
    if (k.tsc) k.tsc[ba] = ts;
    // BCEWithLogitsLoss(reduction="none") over every class (loss.py:247)
    for (int c = 0; c < k.nc; ++c) {
      const float x = ld_any(L.cls, L.cf16, pix * L.ccs + c);
      const float y = c == tc ? ts : 0.0f;
      cls += (fmaxf(x, 0.0f) - x * y) + log1pf(expf(-fabsf(x)));
    }
    if (gi >= 0) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(k.pbox + ba * 4);
      const float tx1 = g.x1 / L.s, ty1 = g.y1 / L.s, tx2 = g.x2 / L.s, ty2 = g.y2 / L.s;  // target_bboxes /= stride
      box = (1.0f - ciou(p[0], p[1], p[2], p[3], tx1, ty1, tx2, ty2)) * ts;
      const float ax = float(gx) + 0.5f, ay = float(gy) + 0.5f;
      const float dist[4] = {ax - tx1, ay - ty1, tx2 - ax, ty2 - ay};  // bbox2dist
      float dsum = 0.0f;
      for (int s = 0; s < 4; ++s) {
        const float tt = fminf(fmaxf(dist[s], 0.0f), (float)(LS_REG - 1) - 0.01f);
        const int tl = (int)tt;
        const float wl = float(tl + 1) - tt, wr = 1.0f - wl;
        float v[LS_REG];
#pragma unroll
        for (int q = 0; q < LS_REG; ++q) v[q] = ld_any(L.box, L.bf16, pix * L.bcs + s * LS_REG + q);
        float mx = v[0];
#pragma unroll
        for (int q = 1; q < LS_REG; ++q) mx = fmaxf(mx, v[q]);
        float se = 0.0f, xl = 0.0f, xr = 0.0f;
#pragma unroll
        for (int q = 0; q < LS_REG; ++q) {
          se += expf(v[q] - mx);
          xl = q == tl ? v[q] : xl;
          xr = q == tl + 1 ? v[q] : xr;
        }
        const float lse = mx + logf(se);
        dsum += (lse - xl) * wl + (lse - xr) * wr;  // cross_entropy(tl) * wl + cross_entropy(tr) * wr
      }
      dfl = (dsum / 4.0f) * ts;
    }
  }
  red[0][t] = box; red[1][t] = cls; red[2][t] = dfl; red[3][t] = ts;
  __syncthreads();
  for (int half = LS_THREADS / 2; half >= 1; half >>= 1) {
    if (t < half) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[j][t] += red[j][t + half];
    }
    __syncthreads();
  }
  if (t < 4) k.part[((int64_t)b * k.nblk + blockIdx.x) * 4 + t] = red[t][0];
}

// one workgroup
__global__ __launch_bounds__(LS_THREADS) void loss_finish_kernel(LossArgs k) {
#pragma clang fp contract(off)
  __shared__ float denom;
  const int t = threadIdx.x;
  for (int b = t; b < k.B; b += LS_THREADS) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int q = 0; q < k.nblk; ++q)
      for (int j = 0; j < 4; ++j) s[j] += k.part[((int64_t)b * k.nblk + q) * 4 + j];
    for (int j = 0; j < 3; ++j) k.per_image[(int64_t)b * 3 + j] = s[j];
    k.tssimg[b] = s[3];
  }
  __syncthreads();  // (the stores above are this workgroup's own: visible after the barrier)
  if (t == 0) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int b = 0; b < k.B; ++b) {
      for (int j = 0; j < 3; ++j) s[j] += k.per_image[(int64_t)b * 3 + j];
      s[3] += k.tssimg[b];
    }
    const float d = fmaxf(s[3], 1.0f);  // target_scores_sum = max(target_scores.sum(), 1)
    denom = d;
    *k.tss = d;
    for (int j = 0; j < 3; ++j) k.loss[j] = (s[j] / d) * k.gain[j];
  }
  __syncthreads();
  const float d = denom;
  for (int i = t; i < k.B * 3; i += LS_THREADS) k.per_image[i] = (k.per_image[i] / d) * k.gain[i % 3];
}

static int64_t ls_words(int64_t B, int64_t A, int64_t M, int64_t* off /* 9 */) {
  const int64_t nblk = cdiv(A, LS_THREADS);
  const int64_t sz[9] = {B * A * 4, B * A, B * A, B * A, B * A, B * M, B * M, B * nblk * 4, B};
  int64_t o = 0;
  for (int i = 0; i < 9; ++i) {
    if (off) off[i] = o;
    o += (sz[i] + 3) & ~int64_t(3);  // every array 16-byte aligned
  }
  return o;
}

}  // namespace ydbl

using namespace ydbl;

extern "C" int64_t ydbl_detect_loss_workspace(int32_t n, int32_t anchors, int32_t max_labels) {
  if (n < 1 || anchors < 1 || max_labels < 0) return -1;
  return ls_words(n, anchors, max_labels, nullptr) * 4;
}

extern "C" int ydbl_detect_loss(const ydbl_loss_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "detect_loss: null descriptor");
  if (d->nl < 1 || d->nl > 3) return fail(YDBL_EINVAL, "detect_loss: nl must be 1..3");
  if (d->nc < 1) return fail(YDBL_EINVAL, "detect_loss: nc < 1");
  if (d->reg_max != LS_REG) return fail(YDBL_EINVAL, "detect_loss: reg_max must be 16");
  if (d->topk < 1 || d->topk > LS_TOPK_MAX) return fail(YDBL_EINVAL, "detect_loss: topk must be 1..16");
  if (d->max_labels < 0) return fail(YDBL_EINVAL, "detect_loss: max_labels < 0");
  if (!d->loss || !d->target_scores_sum || !d->per_image || !d->workspace || (d->max_labels > 0 && !d->gt))
    return fail(YDBL_EINVAL, "detect_loss: null buffer");
  LossArgs k{};
  const int B = d->box[0].n;
  int64_t A = 0;
  for (int l = 0; l < d->nl; ++l) {
    const ydbl_view &bx = d->box[l], &cl = d->cls[l];
    if (!bx.ptr || !cl.ptr) return fail(YDBL_EINVAL, "detect_loss: null level pointer");
    if ((bx.dtype != YDBL_F16 && bx.dtype != YDBL_F32) || (cl.dtype != YDBL_F16 && cl.dtype != YDBL_F32))
      return fail(YDBL_EINVAL, "detect_loss: bad level dtype");
    if (bx.n != B || cl.n != B || B < 1 || bx.h < 1 || bx.w < 1 || cl.h != bx.h || cl.w != bx.w)
      return fail(YDBL_EINVAL, "detect_loss: level shapes disagree or are empty");
    if (bx.c != 4 * LS_REG || cl.c != d->nc || bx.cs < bx.c || cl.cs < cl.c)
      return fail(YDBL_EINVAL, "detect_loss: box view must hold 64 channels, class view nc");
    if (!(d->stride[l] > 0.0f)) return fail(YDBL_EINVAL, "detect_loss: stride must be positive");
    k.lv[l] = LossLevel{bx.ptr, cl.ptr, bx.h, bx.w, bx.cs, cl.cs, bx.dtype == YDBL_F16, cl.dtype == YDBL_F16,
                        (int)A, d->stride[l]};
    A += (int64_t)bx.h * bx.w;
  }
  if (B > 65535 || d->max_labels > 65535) return fail(YDBL_EINVAL, "detect_loss: more than 65535 images or labels per image");
  if ((int64_t)B * A * 4 >= (int64_t)1 << 31) return fail(YDBL_EINVAL, "detect_loss: B * anchors * 4 must stay below 2^31");
  int64_t off[9];
  const int64_t need = ls_words(B, A, d->max_labels, off) * 4;
  if (d->workspace_bytes < need)
    return fail(YDBL_EINVAL, "detect_loss: workspace smaller than ydbl_detect_loss_workspace() = " + std::to_string(need) + " bytes");
  if (reinterpret_cast<uintptr_t>(d->workspace) % 16) return fail(YDBL_EINVAL, "detect_loss: workspace not 16-byte aligned");
  float* ws = reinterpret_cast<float*>(d->workspace);
  k.nl = d->nl; k.nc = d->nc; k.B = B; k.A = (int)A; k.M = d->max_labels; k.topk = d->topk;
  k.nblk = (int)cdiv(A, LS_THREADS);
  k.gt = d->gt;
  k.gain[0] = d->gain_box; k.gain[1] = d->gain_cls; k.gain[2] = d->gain_dfl;
  k.pbox = ws + off[0];
  k.cnt = reinterpret_cast<int*>(ws + off[1]);
  k.owner = reinterpret_cast<int*>(ws + off[2]);
  k.tgt = reinterpret_cast<int*>(ws + off[3]);
  k.am = ws + off[4];
  k.posm = reinterpret_cast<unsigned*>(ws + off[5]);
  k.poso = reinterpret_cast<unsigned*>(ws + off[6]);
  k.part = ws + off[7];
  k.tssimg = ws + off[8];
  k.loss = d->loss; k.tss = d->target_scores_sum; k.per_image = d->per_image;
  k.fg = d->fg; k.tgi = d->target_gt_idx; k.tsc = d->target_score;
  hipStream_t s = as_stream(stream);
  const int64_t n0 = std::max<int64_t>((int64_t)B * A * 4, (int64_t)B * k.M);
  loss_decode_kernel<<<(unsigned)cdiv(n0, LS_THREADS), LS_THREADS, 0, s>>>(k);
  if (k.M > 0) loss_select_kernel<<<dim3(k.M, B), LS_THREADS, 0, s>>>(k);
  loss_resolve_kernel<<<dim3(k.nblk, B), LS_THREADS, 0, s>>>(k);
  loss_terms_kernel<<<dim3(k.nblk, B), LS_THREADS, 0, s>>>(k);
  loss_finish_kernel<<<1, LS_THREADS, 0, s>>>(k);
  return check_launch("ydbl_detect_loss");
}
