// LSKblock's chained depthwise pair (LSKA.py:40-41: dw 5x5, then dw 7x7 dilation 3 on its output), fp16, no
// activation: the fast form of ydbl_dwconv2d_pair_nhwc.  misc.hip's dw_pair_kernel stays the general form (fp32,
// activations, other paddings, larger maps) and the reference this kernel is tested against bit for bit.
//
// dw_pair_kernel gives every thread one (pixel, channel vector) and walks the taps in rolled loops: per tap a wave
// issues 17 vector and 3 LDS instructions for its 8 FMAs per lane -- the bounds tests, the tap counters, eight
// f16 -> f32 conversions and two LDS reads of fp32 taps that are the same for every pixel lane -- and drains
// lgkmcnt once per tap.  Here
//   - a wave owns ONE channel vector and 64 pixels, so the taps are wave-uniform: they are scalar loads of
//     w[tap][c .. c+8) (through the constant address space: after the first store the compiler no longer treats a
//     plain global load as invariant and falls back to per-lane vector loads) and enter the FMAs as scalar operands;
//   - x, and the fp16-rounded first output a1, sit in zero-padded LDS maps ((H+4) x (W+4), (H+18) x (W+18)), one
//     plane per channel vector, so a tap is one 16-byte LDS read at a compile-time offset from the pixel's row
//     address, with no bounds test, and the taps are fully unrolled;
//   - the FMAs read the fp16 halves in place (v_fma_mix_f32: fp16 source, fp32 tap and accumulator): 8 vector and
//     1 LDS instruction per tap;
//   - a tap row's pixels and taps are loaded together and waited for once (12 waits per pixel instead of 74);
//   - workgroups are numbered in XCD-aware order: the four channel groups that share a 128-byte line of x, y0 and
//     y1 run on one XCD and meet in its L2 (bs32 launch 23.5 -> 18.1 us by this alone).
// A padded tap adds fma(0, w, acc), which is acc bit for bit for finite w (acc starts at +0 and round-to-nearest
// never makes it -0), so the fp32 chain per channel -- (ky, kx) order, one rounding per term, bias after the chain,
// a1 rounded to fp16 before the second conv -- is that of the two ydbl_dwconv2d_nhwc launches.
#include "common.hpp"

namespace ydbl {

constexpr int DWF_CV = 2;               // channel vectors (16 channels) per workgroup, as dw_pair_kernel
constexpr int DWF_NT = 1024;            // 16 waves: 8 per channel vector, 64 pixels each
constexpr int DWF_HWMAX = 512;          // = 8 waves x 64 pixels
constexpr int DWF_LDS_MAX = 80 * 1024;  // two workgroups per CU (160 KiB of LDS)

// acc += float(half HI of x) * w, one rounding: v_fma_mix_f32 reads the fp16 half in place, w from an SGPR
template <int HI>
__device__ __forceinline__ float fma_mix(uint32_t x, float w, float acc) {
  if constexpr (HI)
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(x), "s"(w));
  else
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(x), "s"(w));
  return acc;
}

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using cfp = const __attribute__((address_space(4))) float*;  // constant address space: uniform loads are scalar loads

// K x K taps, dilation D, of the padded map `src` (row pitch PW vectors; `src` points at the pixel's first tap);
// w: this wave's 8 channels of tap 0, C floats between taps
template <int K, int D>
__device__ __forceinline__ void dwf_taps(const u32x4* src, int PW, const float* __restrict__ wg, int C, float* acc) {
  const cfp w = (cfp)wg;
#pragma unroll
  for (int ky = 0; ky < K; ++ky) {
    const u32x4* row = src + ky * D * PW;
    float wr[K][8];
    u32x4 xr[K];
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      xr[kx] = row[kx * D];
#pragma unroll
      for (int q = 0; q < 8; ++q) wr[kx][q] = w[(ky * K + kx) * C + q];
    }
    __builtin_amdgcn_sched_barrier(0);  // the row's loads stay together: one wait per row, not one per tap
#pragma unroll
    for (int kx = 0; kx < K; ++kx)
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        acc[2 * h] = fma_mix<0>(xr[kx][h], wr[kx][2 * h], acc[2 * h]);
        acc[2 * h + 1] = fma_mix<1>(xr[kx][h], wr[kx][2 * h + 1], acc[2 * h + 1]);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
}

__global__ __launch_bounds__(DWF_NT) void dw_pair_fast_kernel(DView<const _Float16> x, DView<_Float16> y0,
                                                               DView<_Float16> y1, const float* __restrict__ w0,
                                                               const float* __restrict__ b0,
                                                               const float* __restrict__ w1,
                                                               const float* __restrict__ b1) {
  constexpr int V = 8, CV = DWF_CV, P0 = 2, P1 = 9;  // pads of the 5x5 and the dilated 7x7
  extern __shared__ __align__(16) unsigned char dwf_lds[];
  const int C = y0.c, H = x.h, W = x.w, HW = H * W;
  const int PW0 = W + 2 * P0, PH0 = H + 2 * P0, PW1 = W + 2 * P1, PH1 = H + 2 * P1;
  const int N0 = PH0 * PW0, N1 = PH1 * PW1;      // vectors per plane
  u32x4* sx = reinterpret_cast<u32x4*>(dwf_lds);  // [CV][PH0][PW0]
  u32x4* sa = sx + CV * N0;                       // [CV][PH1][PW1]
  const int cgroups = C / (CV * V);
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int b = bid / cgroups, c0 = (bid % cgroups) * CV * V;
  const int tid = threadIdx.x;
  // x with its zero border, channel vector fastest in the global reads
  for (int i = tid; i < CV * N0; i += DWF_NT) {
    const int cv = i % CV, pp = i / CV;
    const int yy = pp / PW0 - P0, xx = pp % PW0 - P0;
    const bool ok = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const h8 v = vload_sel(x.at(b, ok ? yy : 0, ok ? xx : 0) + c0 + cv * V, x.p, ok);
    sx[cv * N0 + pp] = __builtin_bit_cast(u32x4, v);
  }
  // a1's zero border (its interior is written by phase 1)
  for (int i = tid; i < CV * N1; i += DWF_NT) {
    const int cv = i / N1, pp = i % N1;
    const int yy = pp / PW1 - P1, xx = pp % PW1 - P1;
    if (!(yy >= 0 && yy < H && xx >= 0 && xx < W)) sa[cv * N1 + pp] = u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();
  const int wave = wave_id();
  const int cv = wave / (DWF_NT / 64 / CV);                // wave-uniform channel vector
  const int p = (wave % (DWF_NT / 64 / CV)) * 64 + (tid & 63);
  const int cc = c0 + cv * V;                              // scalar
  const bool live = p < HW;
  const int oy = live ? p / W : 0, ox = live ? p % W : 0;  // idle lanes read pixel 0 and store nothing

  float acc[V];
#pragma unroll
  for (int q = 0; q < V; ++q) acc[q] = 0.f;
  dwf_taps<5, 1>(sx + cv * N0 + oy * PW0 + ox, PW0, w0 + cc, C, acc);
  if (b0) {
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] += b0[cc + q];
  }
  {
    h8 o;
#pragma unroll
    for (int q = 0; q < V; ++q) o[q] = f16_rne(acc[q]);  // the stored y0 is what the second conv reads
    if (live) {
      vstore(y0.at(b, oy, ox) + cc, o);
      sa[cv * N1 + (oy + P1) * PW1 + ox + P1] = __builtin_bit_cast(u32x4, o);
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < V; ++q) acc[q] = 0.f;
  dwf_taps<7, 3>(sa + cv * N1 + oy * PW1 + ox, PW1, w1 + cc, C, acc);
  if (b1) {
#pragma unroll
    for (int q = 0; q < V; ++q) acc[q] += b1[cc + q];
  }
  if (live) {
    h8 o;
#pragma unroll
    for (int q = 0; q < V; ++q) o[q] = f16_rne(acc[q]);
    vstore(y1.at(b, oy, ox) + cc, o);
  }
}

// LDS bytes of the two padded maps of an H x W image
static int64_t dwf_lds_bytes(int H, int W) {
  return (int64_t)DWF_CV * 16 * ((int64_t)(H + 4) * (W + 4) + (int64_t)(H + 18) * (W + 18));
}

// whether a pair that ydbl_dwconv2d_pair_nhwc has found to be the fused 5x5 -> 7x7 dil 3 geometry is this kernel's
bool dw_pair_fast_ok(const ydbl_dwconv_desc* d0, const ydbl_dwconv_desc* d1) {
  const char* e = getenv("YDBL_DW_PAIR_OLD");  // A/B switch, read per launch: 1 = dw_pair_kernel
  if (e && *e == '1') return false;
  return d0->x.dtype == YDBL_F16 && d0->act == YDBL_ACT_NONE && d1->act == YDBL_ACT_NONE && d0->pad == 2 &&
         d1->pad == 9 && d0->x.h * d0->x.w <= DWF_HWMAX && dwf_lds_bytes(d0->x.h, d0->x.w) <= DWF_LDS_MAX &&
         !epi_generic();
}

int dw_pair_fast_launch(const ydbl_dwconv_desc* d0, const ydbl_dwconv_desc* d1, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(dw_pair_fast_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, DWF_LDS_MAX);
  if (attr != hipSuccess) return fail(YDBL_ELAUNCH, std::string("dw_pair: ") + hipGetErrorString(attr));
  const unsigned blocks = (unsigned)(d0->y.n * (d0->y.c / (DWF_CV * 8)));
  const DView<const _Float16> xv{reinterpret_cast<const _Float16*>(d0->x.ptr), d0->x.n, d0->x.h, d0->x.w, d0->x.c,
                                 d0->x.cs};
  dw_pair_fast_kernel<<<blocks, DWF_NT, (size_t)dwf_lds_bytes(d0->x.h, d0->x.w), s>>>(
      xv, dview<_Float16>(d0->y), dview<_Float16>(d1->y), d0->w, d0->bias, d1->w, d1->bias);
  return check_launch("ydbl_dwconv2d_pair_nhwc");
}

}  // namespace ydbl
