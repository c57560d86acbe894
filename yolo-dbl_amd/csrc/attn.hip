// Area attention (AAttn's attention core, U/nn/modules/block.py:1243-1264), head_dim 32, gfx950.
//
// One workgroup = 4 waves = 64 query tokens of one (image, chunk, head); each wave owns 16 queries.  Key / value
// tiles stream through LDS with an online softmax, so the chunk length T is not bounded by LDS.  Both products
// run transposed, which keeps the softmax row on the lane and needs no cross-lane transpose between them:
//
//   S^T[key][q] = sum_d K[key][d] Q[q][d]        A = K tile rows (LDS), B = Q (registers, loaded once)
//   O^T[d][q]   = sum_key V[key][d] P^T[key][q]  A = V^T (LDS),        B = P^T = exp(S^T - m), straight from the
//                                                                          accumulator registers of S^T
//
// The MFMA C/D map (col = lane & 15, row = 4 * (lane >> 4) + reg) puts query q = lane & 15 on the lane for both
// results: the running maximum m, the sum l and the rescale are per-lane scalars, reduced over the four 16-lane
// groups with two shuffles.  The k index of the second product is whatever order the S^T registers come in
// (f16: element 4t+i of lane group g is key 16t + 4g + i of a 32-key step); the V operand is read in that order.
//
//   f16: v_mfma_f32_16x16x32_f16, 64-key tiles, V staged transposed ([d][key]) so a lane's 4 consecutive keys are
//        one 8-byte LDS read; m, l, O in fp32, P rounded to f16 for P V.
//   f32: v_mfma_f32_16x16x4_f32, 32-key tiles, K and V staged as they are ([key][d]); IEEE expf.
//
// The workgroups of query block 0 also write the V channels, re-laid [head*32 + d], as they stage them (the input
// of AAttn.pe): bit copies.
#include "common.hpp"

namespace ydbl {
namespace {

constexpr int HD = 32;  // head_dim (A2C2f asserts c_ % 32 == 0 and uses c_ / 32 heads)
constexpr int BQ = 64;  // queries per workgroup

__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

struct Where {
  int head;
  int64_t pix0;  // first token of this (image, chunk) in pixels of the view
};
__device__ __forceinline__ Where where(int heads, int area, int hw, int T) {
  int z = blockIdx.y;
  const int head = z % heads;
  z /= heads;
  const int chunk = z % area, img = z / area;
  return Where{head, (int64_t)img * hw + (int64_t)chunk * T};
}

__global__ __launch_bounds__(256) void area_attn_f16(DView<const _Float16> qkv, DView<_Float16> y,
                                                     DView<_Float16> vo, int heads, int area, int T, float scale) {
  constexpr int BK = 64, KS = HD + 8, VS = BK + 8;  // row strides in halves: 80 B (16-B reads), 144 B (8-B reads)
  __shared__ __attribute__((aligned(16))) _Float16 Ks[BK * KS];
  __shared__ __attribute__((aligned(16))) _Float16 Vt[HD * VS];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int r16 = lane & 15, g = lane >> 4;
  const Where at = where(heads, area, qkv.h * qkv.w, T);
  const _Float16* base = qkv.p + at.pix0 * qkv.cs + at.head * (3 * HD);
  const int q0 = blockIdx.x * BQ + wave * 16;  // wave-uniform
  const bool wave_on = q0 < T;
  const int qi = q0 + r16;
  const h8 qf = vload(base + (int64_t)min(qi, T - 1) * qkv.cs + 8 * g);  // B[k = d = 8g + j][col = q]

  const int skey = tid >> 2, part = tid & 3;  // staging: one key, 8 of its 32 channels per thread
  const bool write_v = vo.p != nullptr && blockIdx.x == 0;
  h8 kr, vr;
  auto fetch = [&](int kb) {
    const int key = kb + skey;
    const bool ok = key < T;
    const _Float16* p = base + (int64_t)min(key, T - 1) * qkv.cs + part * 8;
    kr = vload(p + HD);
    vr = vload(p + 2 * HD);
    if (ok && write_v) vstore(vo.p + (at.pix0 + key) * vo.cs + at.head * HD + part * 8, vr);
    kr = vsel(kr, ok);
    vr = vsel(vr, ok);  // a masked key's P is 0: its V must be finite
  };

  float m = -INFINITY, l = 0.0f;
  f32x4 o[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};  // O^T[d = 16 dh + 4g + i][q = r16]
  const float sl2 = scale * 1.4426950408889634f;
  fetch(0);
  for (int kb = 0; kb < T; kb += BK) {
    __syncthreads();  // the previous tile has been read
    *reinterpret_cast<h8*>(&Ks[skey * KS + part * 8]) = kr;
#pragma unroll
    for (int j = 0; j < 8; ++j) Vt[(part * 8 + j) * VS + skey] = vr[j];
    __syncthreads();
    if (kb + BK < T) fetch(kb + BK);  // in flight during the MFMAs below
    if (!wave_on) continue;
    f32x4 s[4];
    float tmax = -INFINITY;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const h8 kf = *reinterpret_cast<const h8*>(&Ks[(16 * st + r16) * KS + 8 * g]);
      s[st] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, f32x4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = kb + 16 * st + 4 * g + i < T ? s[st][i] * sl2 : -INFINITY;  // keys past the chunk
        s[st][i] = v;
        tmax = fmaxf(tmax, v);
      }
    }
    const float mn = fmaxf(m, group_max(tmax));  // finite: every tile holds at least one key < T
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    float psum = 0.0f;
#pragma unroll
    for (int st = 0; st < 4; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[st][i] = __builtin_amdgcn_exp2f(s[st][i] - mn);
        psum += s[st][i];
      }
    l = l * alpha + psum;  // this lane's keys only; the four groups are summed at the end (alpha is common to them)
    o[0] *= alpha;
    o[1] *= alpha;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      h8 pf;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) pf[4 * t + i] = (_Float16)s[2 * kk + t][i];
#pragma unroll
      for (int dh = 0; dh < 2; ++dh) {
        const _Float16* vp = &Vt[(16 * dh + r16) * VS + 32 * kk + 4 * g];
        const h4 a0 = *reinterpret_cast<const h4*>(vp), a1 = *reinterpret_cast<const h4*>(vp + 16);
        const h8 vf = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        o[dh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dh], 0, 0, 0);
      }
    }
  }
  if (!wave_on) return;
  const float inv = 1.0f / group_sum(l);
  if (qi >= T) return;  // query rows past the chunk are not stored
  _Float16* yp = y.p + (at.pix0 + qi) * y.cs + at.head * HD + 4 * g;
#pragma unroll
  for (int dh = 0; dh < 2; ++dh) {
    const float v[4] = {o[dh][0] * inv, o[dh][1] * inv, o[dh][2] * inv, o[dh][3] * inv};
    store_f<4>(yp + 16 * dh, v);
  }
}

__global__ __launch_bounds__(256) void area_attn_f32(DView<const float> qkv, DView<float> y, DView<float> vo,
                                                     int heads, int area, int T, float scale) {
  constexpr int BK = 32, RS = HD + 4;  // 144-B rows: 16-B aligned staging writes
  __shared__ __attribute__((aligned(16))) float Ks[BK * RS];
  __shared__ __attribute__((aligned(16))) float Vs[BK * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int r16 = lane & 15, g = lane >> 4;
  const Where at = where(heads, area, qkv.h * qkv.w, T);
  const float* base = qkv.p + at.pix0 * qkv.cs + at.head * (3 * HD);
  const int q0 = blockIdx.x * BQ + wave * 16;  // wave-uniform
  const bool wave_on = q0 < T;
  const int qi = q0 + r16;
  float qf[8];  // B[k = g][col = q] of k-step ss: Q[q][4 ss + g]
  {
    const float* qp = base + (int64_t)min(qi, T - 1) * qkv.cs + g;
#pragma unroll
    for (int ss = 0; ss < 8; ++ss) qf[ss] = qp[4 * ss];
  }

  const int skey = tid >> 3, part = tid & 7;  // staging: one key, 4 of its 32 channels per thread
  const bool write_v = vo.p != nullptr && blockIdx.x == 0;
  f32x4 kr, vr;
  auto fetch = [&](int kb) {
    const int key = kb + skey;
    const bool ok = key < T;
    const float* p = base + (int64_t)min(key, T - 1) * qkv.cs + part * 4;
    kr = vload(p + HD);
    vr = vload(p + 2 * HD);
    if (ok && write_v) vstore(vo.p + (at.pix0 + key) * vo.cs + at.head * HD + part * 4, vr);
    kr = vsel(kr, ok);
    vr = vsel(vr, ok);
  };

  float m = -INFINITY, l = 0.0f;
  f32x4 o[2] = {f32x4{0, 0, 0, 0}, f32x4{0, 0, 0, 0}};
  fetch(0);
  for (int kb = 0; kb < T; kb += BK) {
    __syncthreads();
    *reinterpret_cast<f32x4*>(&Ks[skey * RS + part * 4]) = kr;
    *reinterpret_cast<f32x4*>(&Vs[skey * RS + part * 4]) = vr;
    __syncthreads();
    if (kb + BK < T) fetch(kb + BK);
    if (!wave_on) continue;
    f32x4 s[2];
    float tmax = -INFINITY;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      s[st] = f32x4{0, 0, 0, 0};
      const float* kp = &Ks[(16 * st + r16) * RS + g];
#pragma unroll
      for (int ss = 0; ss < 8; ++ss) s[st] = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[4 * ss], qf[ss], s[st], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = kb + 16 * st + 4 * g + i < T ? s[st][i] * scale : -INFINITY;
        s[st][i] = v;
        tmax = fmaxf(tmax, v);
      }
    }
    const float mn = fmaxf(m, group_max(tmax));
    const float alpha = expf(m - mn);
    m = mn;
    float psum = 0.0f;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[st][i] = expf(s[st][i] - mn);
        psum += s[st][i];
      }
    l = l * alpha + psum;
    o[0] *= alpha;
    o[1] *= alpha;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // k = g of this step is key 16 st + 4g + i: the lane's own P^T register
        const float* vp = &Vs[(16 * st + 4 * g + i) * RS + r16];
#pragma unroll
        for (int dh = 0; dh < 2; ++dh)
          o[dh] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * dh], s[st][i], o[dh], 0, 0, 0);
      }
  }
  if (!wave_on) return;
  const float inv = 1.0f / group_sum(l);
  if (qi >= T) return;
  float* yp = y.p + (at.pix0 + qi) * y.cs + at.head * HD + 4 * g;
#pragma unroll
  for (int dh = 0; dh < 2; ++dh) {
    const float v[4] = {o[dh][0] * inv, o[dh][1] * inv, o[dh][2] * inv, o[dh][3] * inv};
    store_f<4>(yp + 16 * dh, v);
  }
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_area_attn(const ydbl_area_attn_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "area_attn: null descriptor");
  if (check_view(&d->qkv, "area_attn.qkv", true) || check_view(&d->y, "area_attn.y", true)) return YDBL_EINVAL;
  const bool has_v = d->v.ptr != nullptr;
  if (has_v && check_view(&d->v, "area_attn.v", true)) return YDBL_EINVAL;
  if (d->heads < 1 || d->area < 1) return fail(YDBL_EINVAL, "area_attn: heads and area must be >= 1");
  const int C = d->heads * HD;
  if (d->qkv.c != 3 * C) return fail(YDBL_EINVAL, "area_attn: qkv must hold 3 * heads * 32 channels");
  auto fits = [&](const ydbl_view& v) {
    return v.c == C && v.n == d->qkv.n && v.h == d->qkv.h && v.w == d->qkv.w && v.dtype == d->qkv.dtype;
  };
  if (!fits(d->y) || (has_v && !fits(d->v))) return fail(YDBL_EINVAL, "area_attn: y / v must be [n,h,w,heads*32] of qkv's dtype");
  const int64_t hw = (int64_t)d->qkv.h * d->qkv.w;
  if (hw % d->area) return fail(YDBL_EINVAL, "area_attn: h*w is not a multiple of area");
  const int64_t T = hw / d->area, gy = (int64_t)d->qkv.n * d->area * d->heads;
  if (hw > INT32_MAX || gy > 65535) return fail(YDBL_EINVAL, "area_attn: n * area * heads must be <= 65535");
  const dim3 grid((unsigned)cdiv(T, BQ), (unsigned)gy);
  const hipStream_t s = as_stream(stream);
  ydbl_view vnull = d->v;
  if (!has_v) vnull.ptr = nullptr;
  if (d->qkv.dtype == YDBL_F16)
    area_attn_f16<<<grid, 256, 0, s>>>(DView<const _Float16>{(const _Float16*)d->qkv.ptr, d->qkv.n, d->qkv.h, d->qkv.w,
                                                              d->qkv.c, d->qkv.cs},
                                       dview<_Float16>(d->y), dview<_Float16>(vnull), d->heads, d->area, (int)T, d->scale);
  else
    area_attn_f32<<<grid, 256, 0, s>>>(DView<const float>{(const float*)d->qkv.ptr, d->qkv.n, d->qkv.h, d->qkv.w,
                                                          d->qkv.c, d->qkv.cs},
                                       dview<float>(d->y), dview<float>(vnull), d->heads, d->area, (int)T, d->scale);
  return check_launch("ydbl_area_attn");
}
