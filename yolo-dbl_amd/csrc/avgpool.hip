// Global average pool of an NHWC view, the reduction behind Model.embed(): BaseModel._predict_once with embed set
// (U/nn/tasks.py:168-169, adaptive_avg_pool2d(x, (1, 1)).squeeze(-1).squeeze(-1)) -> y[n][c] in the view's dtype.
//
// Memory-bound, every element read once (plain loads: the map was written by the launch before and sits in L2 / the
// Infinity Cache).  An image's h*w pixels are cut into chunks of about AP_BLOCK_BYTES; one 256-thread workgroup per
// (chunk, image).  Its threads cover pixel lanes x channel vectors (16-byte loads: 8 halves / 4 floats, AP_UNROLL in
// flight per thread, the index clamped to the chunk's last pixel instead of a branch around the load); each thread
// adds its pixels in ascending order in fp32, the pixel lanes meet in LDS in a fixed pairwise tree.
//   one chunk  : the workgroup divides by h*w and stores y itself (one launch, no workspace);
//   more chunks: it stores its fp32 partial row to the workspace [n][chunks][c]; a second launch adds an image's
//                partial rows (chunk lanes in ascending order, then the lanes in order) and stores y.
// No floating-point atomics, no arrival order anywhere: the result is a fixed expression tree per (h*w, c, dtype,
// vector or scalar path) -- the chunking never looks at n -- so an image pools to the same bits alone, in any batch
// and on every run.  mean = sum / float(h*w) in fp32, then one round-to-nearest-even to the view's dtype.
// A view that breaks the vector rule (c or cs not a multiple of the vector, pointer not 16-byte aligned) takes the
// same kernel with one-element "vectors".
// Bytes: n*h*w*c*esize read; per image chunks*c*4 written and read again when chunks > 1 (DBL-n at 640^2 fp16:
// 20^2 x 256 ch = 205 KB + 13 KB of partials, 320^2 x 16 ch = 3.3 MB + 13 KB).
#include "common.hpp"

namespace ydbl {

constexpr int AP_THREADS = 256;
constexpr int AP_UNROLL = 4;            // loads in flight per thread
constexpr int AP_BLOCK_BYTES = 16384;   // a workgroup's share of an image: AP_THREADS x AP_UNROLL 16-byte loads
constexpr int AP_MAX_CHUNKS = 256;      // per image (the second launch reads chunks x c floats per image)

// pixels per chunk and chunks per image: a function of (h*w, c, element size) only
static inline void ap_split(int64_t hw, int c, int esize, int64_t* chunk_px, int* chunks) {
  int64_t px = AP_BLOCK_BYTES / ((int64_t)c * esize);
  if (px < 1) px = 1;
  if (cdiv(hw, px) > AP_MAX_CHUNKS) px = cdiv(hw, AP_MAX_CHUNKS);
  *chunk_px = px;
  *chunks = (int)cdiv(hw, px);
}

template <typename T, int VEC>
struct ApLoad {
  static __device__ __forceinline__ void load(const T* p, float* o) { load_f<VEC>(p, o); }
};
template <typename T>
struct ApLoad<T, 1> {
  static __device__ __forceinline__ void load(const T* p, float* o) { o[0] = float(p[0]); }
};

template <typename T>
__device__ __forceinline__ T ap_mean(float sum, float count) {
  const float m = sum / count;
  if constexpr (std::is_same<T, float>::value) return m;
  else return f16_rne(m);
}

// grid (chunks, n).  units = c / VEC channel vectors; g = min(units, 256) of them side by side, pl = 256 / g pixel
// lanes (threads past g * pl idle); more than 256 vectors: the workgroup walks them 256 at a time.
template <typename T, int VEC>
__global__ __launch_bounds__(AP_THREADS) void avgpool_kernel(const T* __restrict__ x, int64_t hw, int c, int cs,
                                                             int64_t chunk_px, int chunks, T* __restrict__ y,
                                                             int64_t y_stride, float* __restrict__ part) {
  __shared__ float red[AP_THREADS * VEC];
  const int k = blockIdx.x, n = blockIdx.y, t = threadIdx.x;
  const int units = c / VEC;
  const int g = min(units, AP_THREADS), pl = AP_THREADS / g;
  const int u = t % g, p = t / g;
  const int64_t lo = (int64_t)k * chunk_px, hi = min(lo + chunk_px, hw);  // lo < hw: chunks = cdiv(hw, chunk_px)
  const T* xi = x + (int64_t)n * hw * cs;
  const float count = (float)hw;
  for (int u0 = 0; u0 < units; u0 += g) {  // (uniform: one trip unless c > 256 vectors)
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0f;
    if (p < pl && u0 + u < units) {
      const T* col = xi + (int64_t)(u0 + u) * VEC;
      for (int64_t px = lo + p; px < hi; px += (int64_t)pl * AP_UNROLL) {
        float v[AP_UNROLL][VEC];
#pragma unroll
        for (int j = 0; j < AP_UNROLL; ++j)
          ApLoad<T, VEC>::load(col + min(px + (int64_t)j * pl, hi - 1) * cs, v[j]);
#pragma unroll
        for (int j = 0; j < AP_UNROLL; ++j) {
          const bool ok = px + (int64_t)j * pl < hi;
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc[e] = ok ? acc[e] + v[j][e] : acc[e];
        }
      }
    }
    if (p < pl) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) red[(p * g + u) * VEC + e] = acc[e];
    }
    __syncthreads();
    // the pixel lanes meet pairwise, lane p taking lane p + half: a fixed tree, log2(pl) steps (a serial walk of
    // pl = 128 lanes by 16 threads was most of the 320^2 x 16-channel launch)
    int half = 1;
    while (half * 2 < pl) half *= 2;
    for (; half >= 1 && pl > 1; half >>= 1) {
      if (p < half && p + half < pl) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) red[(p * g + u) * VEC + e] += red[((p + half) * g + u) * VEC + e];
      }
      __syncthreads();
    }
    for (int e = t; e < g * VEC; e += AP_THREADS) {
      const int ch = u0 * VEC + e;
      if (ch < c) {
        const float s = red[e];
        if (chunks == 1) y[(int64_t)n * y_stride + ch] = ap_mean<T>(s, count);
        else part[((int64_t)n * chunks + k) * c + ch] = s;
      }
    }
    __syncthreads();
  }
}

// grid (cdiv(c, cw), n): cw channels side by side, 256 / cw chunk lanes; lane l adds the partial rows l, l + lanes,
// ... in ascending order, then the lanes are added in order.
template <typename T>
__global__ __launch_bounds__(AP_THREADS) void avgpool_finish_kernel(const float* __restrict__ part, int chunks, int c,
                                                                    int cw, float count, T* __restrict__ y,
                                                                    int64_t y_stride) {
  __shared__ float red[AP_THREADS];
  const int n = blockIdx.y, t = threadIdx.x;
  const int lanes = AP_THREADS / cw, l = t / cw, ch = blockIdx.x * cw + t % cw;
  float s = 0.0f;
  if (ch < c) {
    const float* row = part + (int64_t)n * chunks * c + ch;
    for (int k = l; k < chunks; k += lanes) s += row[(int64_t)k * c];
  }
  red[t] = s;
  __syncthreads();
  if (t < cw && ch < c) {
    float tot = red[t];
    for (int q = 1; q < lanes; ++q) tot += red[q * cw + t];
    y[(int64_t)n * y_stride + ch] = ap_mean<T>(tot, count);
  }
}

static int ap_check(const ydbl_avgpool_desc* d, const char* who) {
  if (!d) return fail(YDBL_EINVAL, std::string(who) + ": null descriptor");
  const ydbl_view& v = d->x;
  if (v.dtype != YDBL_F32 && v.dtype != YDBL_F16) return fail(YDBL_EINVAL, std::string(who) + ": x: bad dtype");
  if (v.n < 1 || v.h < 1 || v.w < 1 || v.c < 1 || v.cs < v.c)
    return fail(YDBL_EINVAL, std::string(who) + ": x: empty view or bad shape");
  if (v.n > 65535) return fail(YDBL_EINVAL, std::string(who) + ": x: more than 65535 images");
  return YDBL_OK;
}

template <typename T>
static void ap_launch(const ydbl_avgpool_desc* d, int64_t hw, int64_t chunk_px, int chunks, hipStream_t s) {
  constexpr int VEC = Vec<T>::N;
  const ydbl_view& v = d->x;
  const T* x = reinterpret_cast<const T*>(v.ptr);
  T* y = reinterpret_cast<T*>(d->y);
  float* part = reinterpret_cast<float*>(d->workspace);
  const bool vec = v.c % VEC == 0 && v.cs % VEC == 0 && reinterpret_cast<uintptr_t>(v.ptr) % 16 == 0;
  const dim3 grid(chunks, v.n);
  if (vec) avgpool_kernel<T, VEC><<<grid, AP_THREADS, 0, s>>>(x, hw, v.c, v.cs, chunk_px, chunks, y, d->y_stride, part);
  else avgpool_kernel<T, 1><<<grid, AP_THREADS, 0, s>>>(x, hw, v.c, v.cs, chunk_px, chunks, y, d->y_stride, part);
  if (chunks > 1) {
    const int cw = v.c <= 16 ? 16 : (v.c <= 32 ? 32 : 64);
    avgpool_finish_kernel<T><<<dim3((unsigned)cdiv(v.c, cw), v.n), AP_THREADS, 0, s>>>(part, chunks, v.c, cw, (float)hw,
                                                                                      y, d->y_stride);
  }
}

}  // namespace ydbl

using namespace ydbl;

extern "C" int64_t ydbl_global_avgpool_workspace(const ydbl_avgpool_desc* d) {
  if (ap_check(d, "global_avgpool_workspace")) return -1;
  int64_t chunk_px;
  int chunks;
  ap_split((int64_t)d->x.h * d->x.w, d->x.c, d->x.dtype == YDBL_F16 ? 2 : 4, &chunk_px, &chunks);
  return chunks > 1 ? (int64_t)d->x.n * chunks * d->x.c * 4 : 0;
}

extern "C" int ydbl_global_avgpool(const ydbl_avgpool_desc* d, void* stream) {
  if (int rc = ap_check(d, "global_avgpool")) return rc;
  if (!d->x.ptr || !d->y) return fail(YDBL_EINVAL, "global_avgpool: null pointer");
  if (d->y_stride < d->x.c) return fail(YDBL_EINVAL, "global_avgpool: y_stride < c");
  const int esize = d->x.dtype == YDBL_F16 ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(d->x.ptr) % esize || reinterpret_cast<uintptr_t>(d->y) % esize)
    return fail(YDBL_EINVAL, "global_avgpool: pointer not aligned to its element");
  const int64_t hw = (int64_t)d->x.h * d->x.w;
  int64_t chunk_px;
  int chunks;
  ap_split(hw, d->x.c, esize, &chunk_px, &chunks);
  if (chunks > 1) {
    const int64_t need = (int64_t)d->x.n * chunks * d->x.c * 4;
    if (!d->workspace || d->workspace_bytes < need)
      return fail(YDBL_EINVAL, "global_avgpool: workspace smaller than ydbl_global_avgpool_workspace(d) = " +
                                   std::to_string(need) + " bytes");
    if (reinterpret_cast<uintptr_t>(d->workspace) % 4) return fail(YDBL_EINVAL, "global_avgpool: workspace not 4-byte aligned");
  }
  if (d->x.dtype == YDBL_F16) ap_launch<_Float16>(d, hw, chunk_px, chunks, as_stream(stream));
  else ap_launch<float>(d, hw, chunk_px, chunks, as_stream(stream));
  return check_launch("ydbl_global_avgpool");
}
