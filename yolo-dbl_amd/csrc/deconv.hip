// ConvTranspose2d(cin, cout, kernel 2, stride 2, pad 0) + bias + activation on NHWC views, gfx950: Proto's upsample
// (U/nn/modules/block.py:87-104).
//
// With kernel == stride no two input pixels meet in an output pixel, so the layer is one GEMM
//   D[m][q * cout + co] = sum_ci X[m][ci] W[q][co][ci],   m = (n, i, j),  q = 2 dy + dx,
// whose four column quarters land on the four output pixels (2i + dy, 2j + dx) of m: a pixel-shuffle store straight
// from the accumulators, no intermediate in memory.  The product runs transposed,
//   D^T[col][m]: A = packed weight rows (16 columns x K), B = X (16 pixels x K),
// so that the MFMA C/D map (col = lane & 15, row = 4 * (lane >> 4) + reg) leaves a lane with output channels of one
// pixel.  Which channel an A row holds is free: in a pair of 16-row tiles, row 4 g + i of tile t holds channel
// 8 g + 4 t + i of the pair's 32, so lane group g ends up with the 8 consecutive channels 8 g .. 8 g + 7 -- one 16-byte
// store per pixel and pair in f16 (two in f32), 64 contiguous bytes per pixel from the four lane groups.
//
//   f16: v_mfma_f32_16x16x32_f16, a lane's 8 consecutive k are one 16-byte load of either operand;
//   f32: v_mfma_f32_16x16x4_f32 (exact fp32 products), four steps per 16-byte load: lane group g holds
//        k = 16 s + 4 g + j and step j multiplies the k-set {16 s + 4 g + j}, the same set for both operands.
//
// One workgroup = 4 waves = PT * 16 pixels; wave w takes the 64-column blocks w, w + 4, ... of the 4 * cout columns,
// so the pixels' K vectors are read once from memory and again from cache by the other waves, and every weight row
// comes from L2 (the whole packed weight is 4 * cout * cin elements).  Both operands go from global memory to the
// MFMA registers; nothing is staged in LDS.  Packed weights: [q][cout][cin] in the view dtype (K contiguous), from
// torch's [cin][cout][2][2] by w.permute(2, 3, 1, 0).
//
// Grid: ceil(n * h * w / (16 * PT)).  Limits: n * 2h * 2w < 2^31 output pixels.
#include "common.hpp"

namespace ydbl {
namespace {

template <typename T> struct DcOp;
template <> struct DcOp<_Float16> {
  static constexpr int KC = 32;  // k per operand load
  using vec = h8;
};
template <> struct DcOp<float> {
  static constexpr int KC = 16;
  using vec = f32x4;
};

template <typename T>
__device__ __forceinline__ f32x4 dc_mfma(const typename DcOp<T>::vec& a, const typename DcOp<T>::vec& b, f32x4 c) {
  if constexpr (std::is_same<T, _Float16>::value) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
    return c;
  }
}

template <typename T, int PT>
__global__ __launch_bounds__(256) void deconv2x2_kernel(DView<const T> x, DView<T> y, const T* __restrict__ wp,
                                                        const float* __restrict__ bias, int cin, int cout, int act) {
  using V = typename DcOp<T>::vec;
  constexpr int KC = DcOp<T>::KC, KL = KC / 4;  // k per lane and load
  const int lane = threadIdx.x & 63, wave = wave_id();
  const int r16 = lane & 15, g = lane >> 4;
  const int64_t M = (int64_t)x.n * x.h * x.w;
  const int64_t m0 = (int64_t)blockIdx.x * (16 * PT);

  const T* xrow[PT];   // this lane's B rows: pixel r16 of each pixel tile, clamped into the map
  int64_t obase[PT];   // element offset of output pixel (2i, 2j) of that pixel; -1: past the map, nothing stored
#pragma unroll
  for (int t = 0; t < PT; ++t) {
    const int64_t m = m0 + 16 * t + r16;
    const int64_t mc = m < M ? m : M - 1;
    xrow[t] = x.p + mc * x.cs + KL * g;
    const int j = int(mc % x.w);
    const int64_t ni = mc / x.w;  // n * h + i
    obase[t] = m < M ? ((ni * 2) * (int64_t)y.w + 2 * j) * y.cs : -1;
  }
  const int ncb = (4 * cout) / 64;  // 64-column blocks (cout % 32 == 0: 4 * cout is a multiple of 128)
  for (int cb = wave; cb < ncb; cb += 4) {
    f32x4 acc[4][PT];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int t = 0; t < PT; ++t) acc[ct][t] = f32x4{0, 0, 0, 0};
    // column = q * cout + co: the packed weight is [4 * cout][cin]; tile ct = 2 pr + t of the block takes the rows
    // 32 pr + 8 (r16 >> 2) + 4 t + (r16 & 3) (see above)
    const T* wrow = wp + ((int64_t)cb * 64 + 8 * (r16 >> 2) + (r16 & 3)) * cin + KL * g;
    for (int k = 0; k < cin; k += KC) {
      V b[PT], a[4];
#pragma unroll
      for (int t = 0; t < PT; ++t) b[t] = *reinterpret_cast<const V*>(xrow[t] + k);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        a[ct] = *reinterpret_cast<const V*>(wrow + (int64_t)(32 * (ct >> 1) + 4 * (ct & 1)) * cin + k);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int t = 0; t < PT; ++t) acc[ct][t] = dc_mfma<T>(a[ct], b[t], acc[ct][t]);
    }
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
      const int col0 = cb * 64 + pr * 32;  // a 32-column pair lies in one quarter (cout % 32 == 0)
      const int q = col0 / cout, co = col0 - q * cout + 8 * g;
      const int64_t qoff = ((int64_t)(q >> 1) * y.w + (q & 1)) * y.cs + co;
      float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (bias) load_f<8>(bias + co, bv);
#pragma unroll
      for (int t = 0; t < PT; ++t) {
        if (obase[t] < 0) continue;
        float v[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = apply_act<T>(acc[2 * pr][t][i] + bv[i], act);
          v[4 + i] = apply_act<T>(acc[2 * pr + 1][t][i] + bv[4 + i], act);
        }
        store_f<8>(y.p + obase[t] + qoff, v);
      }
    }
  }
}

template <typename T>
int launch_deconv(const ydbl_deconv_desc* d, hipStream_t s) {
  const int64_t M = (int64_t)d->x.n * d->x.h * d->x.w;
  DView<const T> x{reinterpret_cast<const T*>(d->x.ptr), d->x.n, d->x.h, d->x.w, d->x.c, d->x.cs};
  DView<T> y = dview<T>(d->y);
  const T* w = reinterpret_cast<const T*>(d->w);
  constexpr int PT = std::is_same<T, _Float16>::value ? 2 : 1;
  deconv2x2_kernel<T, PT><<<(unsigned)cdiv(M, 16 * PT), 256, 0, s>>>(x, y, w, d->bias, d->x.c, d->y.c, d->act);
  return check_launch("ydbl_deconv2x2_nhwc");
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_deconv2x2_nhwc(const ydbl_deconv_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "deconv2x2: null descriptor");
  if (int rc = check_view(&d->x, "deconv2x2 x", true)) return rc;
  if (int rc = check_view(&d->y, "deconv2x2 y", true)) return rc;
  if (!d->w) return fail(YDBL_EINVAL, "deconv2x2: null weights");
  if (d->x.dtype != d->y.dtype) return fail(YDBL_EINVAL, "deconv2x2: x and y must share a dtype");
  if (d->x.c % 32 || d->y.c % 32) return fail(YDBL_EINVAL, "deconv2x2: cin and cout must be multiples of 32");
  if (d->y.n != d->x.n || d->y.h != 2 * d->x.h || d->y.w != 2 * d->x.w)
    return fail(YDBL_EINVAL, "deconv2x2: y must be [n, 2h, 2w, cout]");
  if (d->act < YDBL_ACT_NONE || d->act > YDBL_ACT_SIGMOID) return fail(YDBL_EINVAL, "deconv2x2: bad activation code");
  if (reinterpret_cast<uintptr_t>(d->w) % 16 || (d->bias && reinterpret_cast<uintptr_t>(d->bias) % 16))
    return fail(YDBL_EINVAL, "deconv2x2: weights and bias must be 16-byte aligned");
  if ((int64_t)d->y.n * d->y.h * d->y.w >= (int64_t)1 << 31)
    return fail(YDBL_EINVAL, "deconv2x2: more than 2^31 output pixels");
  if (views_overlap(d->x, d->y)) return fail(YDBL_EINVAL, "deconv2x2: y must not overlap x");
  hipStream_t s = as_stream(stream);
  return d->x.dtype == YDBL_F16 ? launch_deconv<_Float16>(d, s) : launch_deconv<float>(d, s);
}
