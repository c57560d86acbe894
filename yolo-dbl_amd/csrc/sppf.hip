// SPPF's three cascaded 5x5 max-pools (U/nn/modules/block.py:179-198) in one launch, gfx950.
//
// m = MaxPool2d(5, 1, 2) pads with -inf, so y1 = m(x), y2 = m(y1), y3 = m(y2) are the 5x5, 9x9 and 13x13 windowed
// maxima of x, each window clipped at the border of the map -- exactly: a maximum never rounds.  They are computed
// that way, all three from one read of x:
//
//   one workgroup = 256 threads = a tile of TH x TW = 8 x 16 output pixels x CV = 2 channel vectors (16 bytes each:
//   8 halves or 4 floats) of one image;
//   1. the tile with its 6-pixel halo, 20 x 28 pixels, goes to LDS; pixels outside the map are -inf;
//   2. row pass: for each of the 20 rows and 16 output columns the maxima over 5, 9 and 13 columns, nested
//      (m9 extends m5, m13 extends m9: 13 LDS reads for the three);
//   3. column pass: one output pixel and vector per thread, the maxima over 5 rows of the 5-column row maxima, 9 rows
//      of the 9-column ones and 13 rows of the 13-column ones, stored to y1, y2, y3.
//
// LDS: 20*28*2*16 = 17920 B (tile) + 3*20*16*2*16 = 30720 B (row maxima) = 48640 B.  NaN propagates as in torch (a
// NaN in the window wins).  Among equal values (+0 and -0) the one kept may differ from the cascade's; every
// other value has the cascade's bits.
//
// Grid: (tiles, ceil(c / vector / 2), n).  Limits: n <= 65535, c / vector <= 131070; beyond them YDBL_EINVAL.
#include "common.hpp"

#include <math.h>

namespace ydbl {
namespace {

constexpr int TH = 8, TW = 16;  // output tile
constexpr int HALO = 6;         // 13 = 2 * 6 + 1
constexpr int IH = TH + 2 * HALO, IW = TW + 2 * HALO;
constexpr int CV = 2;  // channel vectors per workgroup

template <typename T>
__device__ __forceinline__ typename Vec<T>::type vmax(const typename Vec<T>::type& a, const typename Vec<T>::type& b) {
  typename Vec<T>::type o;
#pragma unroll
  for (int i = 0; i < Vec<T>::N; ++i) o[i] = (b[i] > a[i] || b[i] != b[i]) ? b[i] : a[i];
  return o;
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool5_cascade(DView<const T> x, DView<T> y1, DView<T> y2, DView<T> y3,
                                                        int tiles_x) {
  using V = typename Vec<T>::type;
  constexpr int N = Vec<T>::N;
  __shared__ V in[IH * IW * CV];
  __shared__ V rows[3][IH * TW * CV];
  const int tid = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int cv0 = blockIdx.y * CV, nvec = x.c / N, img = blockIdx.z;
  V ninf;
#pragma unroll
  for (int i = 0; i < N; ++i) ninf[i] = T(-INFINITY);

  for (int it = tid; it < IH * IW * CV; it += 256) {
    const int v = it % CV, px = (it / CV) % IW, py = it / (CV * IW);
    const int gy = ty0 - HALO + py, gx = tx0 - HALO + px;
    const bool ok = gy >= 0 && gy < x.h && gx >= 0 && gx < x.w && cv0 + v < nvec;
    const V val = vload(x.at(img, min(max(gy, 0), x.h - 1), min(max(gx, 0), x.w - 1)) + min(cv0 + v, nvec - 1) * N);
    in[it] = ok ? val : ninf;
  }
  __syncthreads();
  for (int it = tid; it < IH * TW * CV; it += 256) {
    const int v = it % CV, ox = (it / CV) % TW, py = it / (CV * TW);
    const V* p = &in[(py * IW + ox + HALO) * CV + v];  // the window's centre
    V m = p[0];
#pragma unroll
    for (int d = 1; d <= 6; ++d) {
      m = vmax<T>(vmax<T>(m, p[-d * CV]), p[d * CV]);
      if (d == 2) rows[0][it] = m;
      if (d == 4) rows[1][it] = m;
    }
    rows[2][it] = m;
  }
  __syncthreads();
  {  // TH * TW * CV == 256: one output pixel and vector per thread
    const int v = tid % CV, ox = (tid / CV) % TW, oy = tid / (CV * TW);
    const int gy = ty0 + oy, gx = tx0 + ox;
    if (gy >= x.h || gx >= x.w || cv0 + v >= nvec) return;
    const int centre = ((oy + HALO) * TW + ox) * CV + v;
    constexpr int RS = TW * CV;  // one row of the row-maxima buffers
    V m5 = rows[0][centre], m9 = rows[1][centre], m13 = rows[2][centre];
#pragma unroll
    for (int d = 1; d <= 6; ++d) {
      if (d <= 2) m5 = vmax<T>(vmax<T>(m5, rows[0][centre - d * RS]), rows[0][centre + d * RS]);
      if (d <= 4) m9 = vmax<T>(vmax<T>(m9, rows[1][centre - d * RS]), rows[1][centre + d * RS]);
      m13 = vmax<T>(vmax<T>(m13, rows[2][centre - d * RS]), rows[2][centre + d * RS]);
    }
    const int co = (cv0 + v) * N;
    vstore(y1.at(img, gy, gx) + co, m5);
    vstore(y2.at(img, gy, gx) + co, m9);
    vstore(y3.at(img, gy, gx) + co, m13);
  }
}
static_assert(TH * TW * CV == 256, "the column pass maps one item to each thread");

template <typename T>
void launch(const ydbl_maxpool5_desc* d, hipStream_t s) {
  const int vec = Vec<T>::N;
  const int tiles_x = (int)cdiv(d->x.w, TW), tiles_y = (int)cdiv(d->x.h, TH);
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)cdiv(d->x.c / vec, CV), (unsigned)d->x.n);
  maxpool5_cascade<T><<<grid, 256, 0, s>>>(
      DView<const T>{(const T*)d->x.ptr, d->x.n, d->x.h, d->x.w, d->x.c, d->x.cs}, dview<T>(d->y1), dview<T>(d->y2),
      dview<T>(d->y3), tiles_x);
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_maxpool5_cascade(const ydbl_maxpool5_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "maxpool5_cascade: null descriptor");
  if (d->k != 5) return fail(YDBL_EINVAL, "maxpool5_cascade: k must be 5 (SPPF's MaxPool2d(5, 1, 2))");
  if (check_view(&d->x, "maxpool5_cascade.x", true) || check_view(&d->y1, "maxpool5_cascade.y1", true) ||
      check_view(&d->y2, "maxpool5_cascade.y2", true) || check_view(&d->y3, "maxpool5_cascade.y3", true))
    return YDBL_EINVAL;
  const ydbl_view* ys[3] = {&d->y1, &d->y2, &d->y3};
  for (const ydbl_view* y : ys)
    if (y->n != d->x.n || y->h != d->x.h || y->w != d->x.w || y->c != d->x.c || y->dtype != d->x.dtype)
      return fail(YDBL_EINVAL, "maxpool5_cascade: y1, y2, y3 must have x's shape and dtype");
  for (int i = 0; i < 3; ++i) {
    if (views_overlap(d->x, *ys[i])) return fail(YDBL_EINVAL, "maxpool5_cascade: an output overlaps x");
    for (int j = i + 1; j < 3; ++j)
      if (views_overlap(*ys[i], *ys[j])) return fail(YDBL_EINVAL, "maxpool5_cascade: two outputs overlap");
  }
  const int vec = d->x.dtype == YDBL_F16 ? 8 : 4;
  if (d->x.n > 65535 || cdiv(d->x.c / vec, CV) > 65535 ||
      cdiv(d->x.w, TW) * cdiv(d->x.h, TH) > INT32_MAX || (int64_t)d->x.n * d->x.h > INT32_MAX)
    return fail(YDBL_EINVAL, "maxpool5_cascade: n <= 65535, c <= 131070 channel vectors, n * h < 2^31");
  if (d->x.dtype == YDBL_F16) launch<_Float16>(d, as_stream(stream));
  else launch<float>(d, as_stream(stream));
  return check_launch("ydbl_maxpool5_cascade");
}
