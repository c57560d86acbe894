// C2PSA's attention core (Attention.forward without its convs, U/nn/modules/block.py:919-928), key_dim 32,
// head_dim 64, gfx950.
//
// qkv holds, per head, one block of 128 channels: q 0..31 | k 32..63 | v 64..127 (the reference's
// view(B, heads, 2*kd + hd, N).split).  For each (image, head): P = softmax(q k^T * scale) over all N = h*w keys,
// y[token][head*64 + d] = sum_key P[token][key] v[key][d].
//
// The scheme is csrc/attn.hip's (the two files share no code: attn.hip is built for q, k, v of one width, 32):
// one workgroup = 4 waves = 64 query tokens of one (image, head), each wave 16 queries; key / value tiles stream
// through LDS with an online softmax, so N is not bounded by LDS, and both products run transposed so that the
// softmax row stays on the lane:
//
//   S^T[key][q] = sum_d K[key][d] Q[q][d]        A = K tile rows (LDS), B = Q (registers, loaded once)
//   O^T[d][q]   = sum_key V[key][d] P^T[key][q]  A = V^T (LDS),        B = P^T = exp(S^T - m), straight from the
//                                                                          accumulator registers of S^T
//
// The MFMA C/D map (col = lane & 15, row = 4 * (lane >> 4) + reg) puts query q = lane & 15 on the lane for both
// results: the running maximum m, the sum l and the rescale are per-lane scalars, reduced over the four 16-lane
// groups with two shuffles.  The k index of the second product is the order the S^T registers come in (f16: element
// 4t+i of lane group g is key 16t + 4g + i of a 32-key step); the V operand is read in that order.
//
//   f16: v_mfma_f32_16x16x32_f16 -- key_dim 32 is exactly one K step for a 16-key score tile; 64-key tiles, V staged
//        transposed ([d][key]) so a lane's 4 consecutive keys are one 8-byte LDS read; m, l, O in fp32, P rounded
//        to f16 for P V; four 16-row O^T blocks (d = 0..63) per wave.  LDS 5120 B (K) + 9216 B (V^T).
//   f32: v_mfma_f32_16x16x4_f32, 32-key tiles, K and V staged as they are ([key][d]); IEEE expf.
//        LDS 4608 B (K) + 8704 B (V).
//
// The workgroups of query tile 0 also write the V channels, re-laid [head*64 + d], as they stage them (the input of
// Attention.pe): bit copies.  Keys past N are masked (score -inf, V zero), query rows past N are not stored.
//
// Grid: (ceil(N / 64), heads, n).  Limits: heads <= 65535, n <= 65535, N = h*w < 2^31; beyond them YDBL_EINVAL.
#include "common.hpp"

namespace ydbl {
namespace {

constexpr int KD = 32;              // key_dim
constexpr int VD = 64;              // head_dim
constexpr int HC = 2 * KD + VD;     // channels of one head in qkv
constexpr int BQ = 64;              // queries per workgroup
constexpr int NB = VD / 16;         // 16-row blocks of O^T

__device__ __forceinline__ float group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

__global__ __launch_bounds__(256) void psa_attn_f16(DView<const _Float16> qkv, DView<_Float16> y, DView<_Float16> vo,
                                                    int N, float scale) {
  constexpr int BK = 64, KS = KD + 8, VS = BK + 8;  // row strides in halves: 80 B (16-B reads), 144 B (8-B reads)
  __shared__ __attribute__((aligned(16))) _Float16 Ks[BK * KS];
  __shared__ __attribute__((aligned(16))) _Float16 Vt[VD * VS];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int r16 = lane & 15, g = lane >> 4;
  const int head = blockIdx.y;
  const int64_t pix0 = (int64_t)blockIdx.z * N;  // first token of this image in pixels of the view
  const _Float16* base = qkv.p + pix0 * qkv.cs + head * HC;
  const int q0 = blockIdx.x * BQ + wave * 16;  // wave-uniform
  const bool wave_on = q0 < N;
  const int qi = q0 + r16;
  const h8 qf = vload(base + (int64_t)min(qi, N - 1) * qkv.cs + 8 * g);  // B[k = d = 8g + j][col = q]

  const int skey = tid >> 2, part = tid & 3;  // staging: one key per 4 threads, 8 of its K and 2 x 8 of its V channels
  const bool write_v = vo.p != nullptr && blockIdx.x == 0;
  h8 kr, vr0, vr1;
  auto fetch = [&](int kb) {
    const int key = kb + skey;
    const bool ok = key < N;
    const _Float16* p = base + (int64_t)min(key, N - 1) * qkv.cs + part * 8;
    kr = vload(p + KD);
    vr0 = vload(p + 2 * KD);
    vr1 = vload(p + 2 * KD + 32);
    if (ok && write_v) {
      _Float16* o = vo.p + (pix0 + key) * vo.cs + head * VD + part * 8;
      vstore(o, vr0);
      vstore(o + 32, vr1);
    }
    kr = vsel(kr, ok);
    vr0 = vsel(vr0, ok);  // a masked key's P is 0: its V must be finite
    vr1 = vsel(vr1, ok);
  };

  float m = -INFINITY, l = 0.0f;
  f32x4 o[NB];  // O^T[d = 16 dh + 4g + i][q = r16]
#pragma unroll
  for (int dh = 0; dh < NB; ++dh) o[dh] = f32x4{0, 0, 0, 0};
  const float sl2 = scale * 1.4426950408889634f;
  fetch(0);
  for (int kb = 0; kb < N; kb += BK) {
    __syncthreads();  // the previous tile has been read
    *reinterpret_cast<h8*>(&Ks[skey * KS + part * 8]) = kr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Vt[(part * 8 + j) * VS + skey] = vr0[j];
      Vt[(32 + part * 8 + j) * VS + skey] = vr1[j];
    }
    __syncthreads();
    if (kb + BK < N) fetch(kb + BK);  // in flight during the MFMAs below
    if (!wave_on) continue;
    f32x4 s[4];
    float tmax = -INFINITY;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const h8 kf = *reinterpret_cast<const h8*>(&Ks[(16 * st + r16) * KS + 8 * g]);
      s[st] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, f32x4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = kb + 16 * st + 4 * g + i < N ? s[st][i] * sl2 : -INFINITY;  // keys past the map
        s[st][i] = v;
        tmax = fmaxf(tmax, v);
      }
    }
    const float mn = fmaxf(m, group_max(tmax));  // finite: every tile holds at least one key < N
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
#pragma unroll
    for (int dh = 0; dh < NB; ++dh) o[dh] *= alpha;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      h8 pf;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) pf[4 * t + i] = (_Float16)s[2 * kk + t][i];
#pragma unroll
      for (int dh = 0; dh < NB; ++dh) {
        const _Float16* vp = &Vt[(16 * dh + r16) * VS + 32 * kk + 4 * g];
        const h4 a0 = *reinterpret_cast<const h4*>(vp), a1 = *reinterpret_cast<const h4*>(vp + 16);
        const h8 vf = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        o[dh] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[dh], 0, 0, 0);
      }
    }
  }
  if (!wave_on) return;
  const float inv = 1.0f / group_sum(l);
  if (qi >= N) return;  // query rows past the map are not stored
  _Float16* yp = y.p + (pix0 + qi) * y.cs + head * VD + 4 * g;
#pragma unroll
  for (int dh = 0; dh < NB; ++dh) {
    const float v[4] = {o[dh][0] * inv, o[dh][1] * inv, o[dh][2] * inv, o[dh][3] * inv};
    store_f<4>(yp + 16 * dh, v);
  }
}

__global__ __launch_bounds__(256) void psa_attn_f32(DView<const float> qkv, DView<float> y, DView<float> vo, int N,
                                                    float scale) {
  constexpr int BK = 32, RK = KD + 4, RV = VD + 4;  // 144-B and 272-B rows: 16-B aligned staging writes
  __shared__ __attribute__((aligned(16))) float Ks[BK * RK];
  __shared__ __attribute__((aligned(16))) float Vs[BK * RV];
  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int r16 = lane & 15, g = lane >> 4;
  const int head = blockIdx.y;
  const int64_t pix0 = (int64_t)blockIdx.z * N;
  const float* base = qkv.p + pix0 * qkv.cs + head * HC;
  const int q0 = blockIdx.x * BQ + wave * 16;  // wave-uniform
  const bool wave_on = q0 < N;
  const int qi = q0 + r16;
  float qf[8];  // B[k = g][col = q] of k-step ss: Q[q][4 ss + g]
  {
    const float* qp = base + (int64_t)min(qi, N - 1) * qkv.cs + g;
#pragma unroll
    for (int ss = 0; ss < 8; ++ss) qf[ss] = qp[4 * ss];
  }

  const int skey = tid >> 3, part = tid & 7;  // staging: one key per 8 threads, 4 of its K and 2 x 4 of its V channels
  const bool write_v = vo.p != nullptr && blockIdx.x == 0;
  f32x4 kr, vr0, vr1;
  auto fetch = [&](int kb) {
    const int key = kb + skey;
    const bool ok = key < N;
    const float* p = base + (int64_t)min(key, N - 1) * qkv.cs + part * 4;
    kr = vload(p + KD);
    vr0 = vload(p + 2 * KD);
    vr1 = vload(p + 2 * KD + 32);
    if (ok && write_v) {
      float* o = vo.p + (pix0 + key) * vo.cs + head * VD + part * 4;
      vstore(o, vr0);
      vstore(o + 32, vr1);
    }
    kr = vsel(kr, ok);
    vr0 = vsel(vr0, ok);
    vr1 = vsel(vr1, ok);
  };

  float m = -INFINITY, l = 0.0f;
  f32x4 o[NB];
#pragma unroll
  for (int dh = 0; dh < NB; ++dh) o[dh] = f32x4{0, 0, 0, 0};
  fetch(0);
  for (int kb = 0; kb < N; kb += BK) {
    __syncthreads();
    *reinterpret_cast<f32x4*>(&Ks[skey * RK + part * 4]) = kr;
    *reinterpret_cast<f32x4*>(&Vs[skey * RV + part * 4]) = vr0;
    *reinterpret_cast<f32x4*>(&Vs[skey * RV + 32 + part * 4]) = vr1;
    __syncthreads();
    if (kb + BK < N) fetch(kb + BK);
    if (!wave_on) continue;
    f32x4 s[2];
    float tmax = -INFINITY;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      s[st] = f32x4{0, 0, 0, 0};
      const float* kp = &Ks[(16 * st + r16) * RK + g];
#pragma unroll
      for (int ss = 0; ss < 8; ++ss) s[st] = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[4 * ss], qf[ss], s[st], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = kb + 16 * st + 4 * g + i < N ? s[st][i] * scale : -INFINITY;
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
#pragma unroll
    for (int dh = 0; dh < NB; ++dh) o[dh] *= alpha;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // k = g of this step is key 16 st + 4g + i: the lane's own P^T register
        const float* vp = &Vs[(16 * st + 4 * g + i) * RV + r16];
#pragma unroll
        for (int dh = 0; dh < NB; ++dh)
          o[dh] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * dh], s[st][i], o[dh], 0, 0, 0);
      }
  }
  if (!wave_on) return;
  const float inv = 1.0f / group_sum(l);
  if (qi >= N) return;
  float* yp = y.p + (pix0 + qi) * y.cs + head * VD + 4 * g;
#pragma unroll
  for (int dh = 0; dh < NB; ++dh) {
    const float v[4] = {o[dh][0] * inv, o[dh][1] * inv, o[dh][2] * inv, o[dh][3] * inv};
    store_f<4>(yp + 16 * dh, v);
  }
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_psa_attn(const ydbl_psa_attn_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "psa_attn: null descriptor");
  if (check_view(&d->qkv, "psa_attn.qkv", true) || check_view(&d->y, "psa_attn.y", true)) return YDBL_EINVAL;
  const bool has_v = d->v.ptr != nullptr;
  if (has_v && check_view(&d->v, "psa_attn.v", true)) return YDBL_EINVAL;
  if (d->key_dim != KD || d->head_dim != VD)
    return fail(YDBL_EINVAL, "psa_attn: the kernel is built for key_dim 32 and head_dim 64");
  if (d->heads < 1 || d->heads > 65535) return fail(YDBL_EINVAL, "psa_attn: heads must be in 1..65535");
  if (d->qkv.c != (int64_t)d->heads * HC) return fail(YDBL_EINVAL, "psa_attn: qkv must hold heads * 128 channels");
  auto fits = [&](const ydbl_view& v) {
    return v.c == d->heads * VD && v.n == d->qkv.n && v.h == d->qkv.h && v.w == d->qkv.w && v.dtype == d->qkv.dtype;
  };
  if (!fits(d->y) || (has_v && !fits(d->v)))
    return fail(YDBL_EINVAL, "psa_attn: y / v must be [n,h,w,heads*64] of qkv's dtype");
  if (views_overlap(d->qkv, d->y) || (has_v && (views_overlap(d->qkv, d->v) || views_overlap(d->y, d->v))))
    return fail(YDBL_EINVAL, "psa_attn: y and v must not overlap qkv or each other");
  const int64_t N = (int64_t)d->qkv.h * d->qkv.w;
  if (N > INT32_MAX || d->qkv.n > 65535) return fail(YDBL_EINVAL, "psa_attn: h * w < 2^31 and n <= 65535");
  const dim3 grid((unsigned)cdiv(N, BQ), (unsigned)d->heads, (unsigned)d->qkv.n);
  const hipStream_t s = as_stream(stream);
  ydbl_view vnull = d->v;
  if (!has_v) vnull.ptr = nullptr;
  if (d->qkv.dtype == YDBL_F16)
    psa_attn_f16<<<grid, 256, 0, s>>>(DView<const _Float16>{(const _Float16*)d->qkv.ptr, d->qkv.n, d->qkv.h, d->qkv.w,
                                                             d->qkv.c, d->qkv.cs},
                                      dview<_Float16>(d->y), dview<_Float16>(vnull), (int)N, d->scale);
  else
    psa_attn_f32<<<grid, 256, 0, s>>>(DView<const float>{(const float*)d->qkv.ptr, d->qkv.n, d->qkv.h, d->qkv.w,
                                                         d->qkv.c, d->qkv.cs},
                                      dview<float>(d->y), dview<float>(vnull), (int)N, d->scale);
  return check_launch("ydbl_psa_attn");
}
