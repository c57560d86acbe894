// The gradient of the detection loss (include/ydbl.h, ydbl_detect_loss_grad): what autograd computes behind
// v8DetectionLoss.__call__ (U/utils/loss.py:206-260) for the level logits, given the assignment csrc/loss.hip wrote
// (a constant in the reference, :233-243).  One launch, a streaming kernel: per anchor it reads the nc class logits
// (and the 64 box logits of a foreground anchor only) and writes 64 + nc gradients, each word once.
//
// A workgroup owns LG_TILE consecutive anchors of one image and walks them twice:
//   class  one lane per anchor, its groups of 8 classes in turn: sigmoid(x) - t.  The foreground flags go to LDS.
//   box    8 lanes per anchor, 8 anchors per wave instruction, 8 channels per lane (one 16-byte access in fp16, two
//          in fp32).  A wave whose 8 anchors hold no foreground stores zeros and loads nothing.  In a wave that holds
//          one, the 8 lanes of the anchor share the work: a side's 16 bins sit in two neighbouring lanes (one
//          xor-shuffle for the softmax), the four distances meet by shuffles and every lane evaluates the CIoU
//          derivative of its own side -- no lane loops over an anchor alone, so a foreground anchor costs its wave
//          one pass of ~200 VALU instructions, not 64 x that.
// The kernel is bound by load latency before it is by bytes (a wave moves ~1 KiB per round trip), so the class pass
// issues its assignment and logit loads together and the box pass reads its flags from LDS: a wave without foreground
// then only streams stores.
// A whole 8-channel group is moved with 16-byte accesses whatever the pitch (element-aligned vector types, below),
// the nc % 8 tail element by element.  All arithmetic fp32 with contraction off, so every pitch and dtype route
// gives the same bits.
// Bytes (DBL-n 640^2, B = 32, nc = 3, fp16 in and out): B x 8400 x (3 x 2 + 67 x 2) B = 37.6 MB + the assignment
// (3 words per anchor, 3.2 MB); reading every box logit as well would make it 72 MB.  Measured: DESIGN.md §4.
#include <math.h>

#include "common.hpp"

namespace ydbl {

constexpr int LG_THREADS = 256;
constexpr int LG_TILE = 256;  // anchors per workgroup
constexpr int LG_REG = 16;    // reg_max

struct GradLevel {
  const void* box; const void* cls; void* gbox; void* gcls;
  int h, w, a0;
  int bcs, ccs, gbcs, gccs;  // channel pitches
  int bf16, cf16, gbf16, gcf16;
  float s;
};

struct GradArgs {
  GradLevel lv[3];
  int nl, nc, B, A, M;
  const float* gt;
  const int* fg; const int* tgi; const float* tsc; const float* tss; const float* grad_scale;
  float batch_scale;
  float gain[3];
};

// 16-byte vectors that promise element alignment only: a view's pixels may start anywhere (pitch 64 + nc), and gfx950
// takes global_load / global_store_dwordx4 at any element-aligned address -- hipcc emits them for these types
typedef h8 h8u __attribute__((aligned(2)));
typedef f32x4 f4u __attribute__((aligned(4)));

// n <= 8 channels at element index i of a view as fp32; 16-byte loads when the group is whole
__device__ __forceinline__ void load8(const void* p, int f16, int64_t i, int n, float (&v)[8]) {
  if (f16) {
    const _Float16* q = reinterpret_cast<const _Float16*>(p) + i;
    if (n == 8) {
      const h8 u = *reinterpret_cast<const h8u*>(q);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = float(u[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = j < n ? float(q[j]) : 0.0f;
    }
  } else {
    const float* q = reinterpret_cast<const float*>(p) + i;
    if (n == 8) {
      const f32x4 u0 = *reinterpret_cast<const f4u*>(q), u1 = *reinterpret_cast<const f4u*>(q + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = u0[j];
        v[j + 4] = u1[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = j < n ? q[j] : 0.0f;
    }
  }
}

// the same for a store; the one rounding to fp16 happens here
__device__ __forceinline__ void store8(void* p, int f16, int64_t i, int n, const float (&v)[8]) {
  if (f16) {
    _Float16* q = reinterpret_cast<_Float16*>(p) + i;
    if (n == 8) {
      h8 u;
#pragma unroll
      for (int j = 0; j < 8; ++j) u[j] = f16_rne(v[j]);
      *reinterpret_cast<h8u*>(q) = u;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < n) q[j] = f16_rne(v[j]);
    }
  } else {
    float* q = reinterpret_cast<float*>(p) + i;
    if (n == 8) {
      *reinterpret_cast<f4u*>(q) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f4u*>(q + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < n) q[j] = v[j];
    }
  }
}

// anchor a of image b -> level, cell; returns the pixel index inside the level's [B][h][w] map
__device__ __forceinline__ int64_t grad_row(const GradArgs& k, int b, int a, int& l, int& gx, int& gy) {
  l = 0;
  if (k.nl > 1 && a >= k.lv[1].a0) l = 1;
  if (k.nl > 2 && a >= k.lv[2].a0) l = 2;
  const int r = a - k.lv[l].a0;
  gy = r / k.lv[l].w;
  gx = r - gy * k.lv[l].w;
  return ((int64_t)b * k.lv[l].h + gy) * k.lv[l].w + gx;
}

// d CIoU / d (x1, y1, x2, y2) of the predicted box a against the target b: bbox_iou(xywh=False, CIoU=True),
// U/utils/metrics.py:102-130, with alpha a constant (:128-129)
__device__ __forceinline__ void ciou_grad(float ax1, float ay1, float ax2, float ay2, float bx1, float by1, float bx2,
                                          float by2, float (&g)[4]) {
#pragma clang fp contract(off)
  const float eps = 1e-7f;
  const float w1 = ax2 - ax1, h1 = ay2 - ay1 + eps;
  const float w2 = bx2 - bx1, h2 = by2 - by1 + eps;
  const float iwr = fminf(ax2, bx2) - fmaxf(ax1, bx1), ihr = fminf(ay2, by2) - fmaxf(ay1, by1);
  const float iw = fmaxf(iwr, 0.0f), ih = fmaxf(ihr, 0.0f);
  const float inter = iw * ih;
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
  // v through atan(w1 / h1): dv/dw1, dv/dh1
  const float q = w1 * w1 + h1 * h1;
  const float dv_w = -0.8105694691387022f * da * (h1 / q);  // 8 / pi^2
  const float dv_h = 0.8105694691387022f * da * (w1 / q);
  // per coordinate: d inter, d union, d c2, d rho2, d v
  const float live_w = iwr >= 0.0f ? 1.0f : 0.0f, live_h = ihr >= 0.0f ? 1.0f : 0.0f;
  const float di[4] = {ax1 >= bx1 ? -live_w * ih : 0.0f, ay1 >= by1 ? -live_h * iw : 0.0f,
                       ax2 <= bx2 ? live_w * ih : 0.0f, ay2 <= by2 ? live_h * iw : 0.0f};
  const float dwh[4] = {-h1, -w1, h1, w1};  // d (w1 * h1)
  const float dc[4] = {ax1 <= bx1 ? -2.0f * cw : 0.0f, ay1 <= by1 ? -2.0f * ch : 0.0f,
                       ax2 >= bx2 ? 2.0f * cw : 0.0f, ay2 >= by2 ? 2.0f * ch : 0.0f};
  const float dr[4] = {-dx / 2.0f, -dy / 2.0f, -dx / 2.0f, -dy / 2.0f};
  const float dv[4] = {-dv_w, -dv_h, dv_w, dv_h};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float du = dwh[j] - di[j];
    const float diou = (di[j] * uni - inter * du) / (uni * uni);
    const float dpen = (dr[j] * c2 - rho2 * dc[j]) / (c2 * c2);
    g[j] = diou - (dpen + alpha * dv[j]);
  }
}

// grid (tiles of LG_TILE anchors, B)
__global__ __launch_bounds__(LG_THREADS) void loss_grad_kernel(GradArgs k) {
#pragma clang fp contract(off)
  __shared__ int s_fg[LG_TILE];
  const int t = threadIdx.x, b = blockIdx.y;
  const int a0 = blockIdx.x * LG_TILE;
  const float S = *k.tss;
  const float K = (k.grad_scale ? *k.grad_scale : 1.0f) * k.batch_scale;
  const float kbox = K * k.gain[0] / S, kcls = K * k.gain[1] / S, kdfl = K * k.gain[2] / S;

  // ---- class: one lane per anchor.  The assignment words and the first class logits are independent loads: one
  // round trip; the flags stay in LDS for the box pass, which then waits for no load in a wave without foreground.
  {
    const int a = a0 + t;
    const bool valid = a < k.A;
    const int64_t ba = (int64_t)b * k.A + (valid ? a : 0);
    int l = 0, gx = 0, gy = 0;
    const int64_t pix = grad_row(k, b, valid ? a : 0, l, gx, gy);
    const GradLevel& L = k.lv[l];
    const bool fg = valid && k.fg[ba] != 0;
    const float w = k.tsc[ba];
    const int gi = k.tgi[ba];
    s_fg[t] = fg;
    const int groups = (k.nc + 7) >> 3, nmax = min(k.nc, 8);
    int tc = -1;
#pragma unroll 1
    for (int grp = 0; grp < groups; ++grp) {  // (uniform)
      const int c0 = grp * 8, n = min(8, k.nc - c0);
      float x[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, g[8];
      if (valid) load8(L.cls, L.cf16, pix * L.ccs + c0, n, x);
      if (grp == 0 && fg) tc = min(max((int)k.gt[((int64_t)b * k.M + gi) * 5], 0), k.nc - 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        g[j] = 0.0f;
        if (j < nmax) {  // (uniform: nc = 3 costs three sigmoids, not eight)
          const float sg = 1.0f / (1.0f + expf(-x[j]));
          g[j] = kcls * (sg - (c0 + j == tc ? w : 0.0f));
        }
      }
      if (valid) store8(L.gcls, L.gcf16, pix * L.gccs + c0, n, g);
    }
  }
  __syncthreads();

  // ---- box: 8 lanes per anchor
  const int sub = t & 7, side = sub >> 1, half = sub & 1;
  const int lane0 = (t & 63) & ~7;
#pragma unroll 1
  for (int it = 0; it < LG_TILE / (LG_THREADS / 8); ++it) {
    const int r = it * (LG_THREADS / 8) + (t >> 3);
    const int a = a0 + r;
    const bool valid = a < k.A;
    const bool fg = s_fg[r] != 0;  // (0 for a row past the end)
    int l = 0, gx = 0, gy = 0;
    int64_t pix = 0;
    if (valid) pix = grad_row(k, b, a, l, gx, gy);
    const GradLevel& L = k.lv[l];
    float g[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (__any(fg)) {  // (wave-uniform)
      float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      if (fg) load8(L.box, L.bf16, pix * L.bcs + sub * 8, 8, z);
      float m = z[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) m = fmaxf(m, z[j]);
      m = fmaxf(m, __shfl_xor(m, 1));
      float p[8], sum = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = expf(z[j] - m);
        sum += p[j];
      }
      sum += __shfl_xor(sum, 1);
      float d = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = p[j] / sum;
        d += p[j] * float(half * 8 + j);
      }
      d += __shfl_xor(d, 1);
      const float dl = __shfl(d, lane0), dt = __shfl(d, lane0 + 2), dr = __shfl(d, lane0 + 4),
                  db = __shfl(d, lane0 + 6);
      if (fg) {
        const int64_t ba = (int64_t)b * k.A + a;
        const float w = k.tsc[ba];
        const float* lab = k.gt + ((int64_t)b * k.M + k.tgi[ba]) * 5;
        const float tx1 = lab[1] / L.s, ty1 = lab[2] / L.s, tx2 = lab[3] / L.s, ty2 = lab[4] / L.s;
        const float ax = float(gx) + 0.5f, ay = float(gy) + 0.5f;
        float gc[4];
        ciou_grad(ax - dl, ay - dt, ax + dr, ay + db, tx1, ty1, tx2, ty2, gc);
        // d CIoU / d d_s: the left and top distances enter with a minus sign
        const float gci = side == 0 ? -gc[0] : side == 1 ? -gc[1] : side == 2 ? gc[2] : gc[3];
        const float dist = side == 0 ? ax - tx1 : side == 1 ? ay - ty1 : side == 2 ? tx2 - ax : ty2 - ay;  // bbox2dist
        const float tt = fminf(fmaxf(dist, 0.0f), (float)(LG_REG - 1) - 0.01f);
        const int tl = (int)tt;
        const float wl = float(tl + 1) - tt, wr = 1.0f - wl;
        const float cb = kbox * w * (-gci), cd = kdfl * w / 4.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int bin = half * 8 + j;
          const float hit = bin == tl ? wl : bin == tl + 1 ? wr : 0.0f;
          g[j] = cb * (p[j] * (float(bin) - d)) + cd * (p[j] - hit);
        }
      }
    }
    if (valid) store8(L.gbox, L.gbf16, pix * L.gbcs + sub * 8, 8, g);
  }
}

static bool lg_dtype(const ydbl_view& v) { return v.dtype == YDBL_F16 || v.dtype == YDBL_F32; }
static bool lg_same_shape(const ydbl_view& g, const ydbl_view& x) {
  return g.n == x.n && g.h == x.h && g.w == x.w && g.c == x.c && g.cs >= g.c;
}

}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_detect_loss_grad(const ydbl_loss_grad_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "detect_loss_grad: null descriptor");
  if (d->nl < 1 || d->nl > 3) return fail(YDBL_EINVAL, "detect_loss_grad: nl must be 1..3");
  if (d->nc < 1) return fail(YDBL_EINVAL, "detect_loss_grad: nc < 1");
  if (d->reg_max != LG_REG) return fail(YDBL_EINVAL, "detect_loss_grad: reg_max must be 16");
  if (d->max_labels < 0) return fail(YDBL_EINVAL, "detect_loss_grad: max_labels < 0");
  if (!d->fg || !d->target_gt_idx || !d->target_score || !d->target_scores_sum || (d->max_labels > 0 && !d->gt))
    return fail(YDBL_EINVAL, "detect_loss_grad: null buffer");
  GradArgs k{};
  const int B = d->box[0].n;
  int64_t A = 0;
  for (int l = 0; l < d->nl; ++l) {
    const ydbl_view &bx = d->box[l], &cl = d->cls[l], &gb = d->gbox[l], &gc = d->gcls[l];
    if (!bx.ptr || !cl.ptr) return fail(YDBL_EINVAL, "detect_loss_grad: null level pointer");
    if (!gb.ptr || !gc.ptr) return fail(YDBL_EINVAL, "detect_loss_grad: null gradient view");
    if (!lg_dtype(bx) || !lg_dtype(cl)) return fail(YDBL_EINVAL, "detect_loss_grad: bad level dtype");
    if (!lg_dtype(gb) || !lg_dtype(gc)) return fail(YDBL_EINVAL, "detect_loss_grad: bad gradient dtype");
    if (bx.n != B || cl.n != B || B < 1 || bx.h < 1 || bx.w < 1 || cl.h != bx.h || cl.w != bx.w)
      return fail(YDBL_EINVAL, "detect_loss_grad: level shapes disagree or are empty");
    if (bx.c != 4 * LG_REG || cl.c != d->nc || bx.cs < bx.c || cl.cs < cl.c)
      return fail(YDBL_EINVAL, "detect_loss_grad: box view must hold 64 channels, class view nc");
    if (!lg_same_shape(gb, bx) || !lg_same_shape(gc, cl))
      return fail(YDBL_EINVAL, "detect_loss_grad: gradient view shapes disagree with the inputs");
    if (!(d->stride[l] > 0.0f)) return fail(YDBL_EINVAL, "detect_loss_grad: stride must be positive");
    k.lv[l] = GradLevel{bx.ptr, cl.ptr, gb.ptr, gc.ptr, bx.h, bx.w, (int)A, bx.cs, cl.cs, gb.cs, gc.cs,
                        bx.dtype == YDBL_F16, cl.dtype == YDBL_F16, gb.dtype == YDBL_F16, gc.dtype == YDBL_F16,
                        d->stride[l]};
    A += (int64_t)bx.h * bx.w;
  }
  if (B > 65535) return fail(YDBL_EINVAL, "detect_loss_grad: more than 65535 images");
  if ((int64_t)B * A >= (int64_t)1 << 31) return fail(YDBL_EINVAL, "detect_loss_grad: B * anchors must stay below 2^31");
  k.nl = d->nl; k.nc = d->nc; k.B = B; k.A = (int)A; k.M = d->max_labels;
  k.gt = d->gt;
  k.fg = d->fg; k.tgi = d->target_gt_idx; k.tsc = d->target_score; k.tss = d->target_scores_sum;
  k.grad_scale = d->grad_scale;
  k.batch_scale = d->batch_scale;
  k.gain[0] = d->gain_box; k.gain[1] = d->gain_cls; k.gain[2] = d->gain_dfl;
  loss_grad_kernel<<<dim3((unsigned)cdiv(A, LG_TILE), B), LG_THREADS, 0, as_stream(stream)>>>(k);
  return check_launch("ydbl_detect_loss_grad");
}
