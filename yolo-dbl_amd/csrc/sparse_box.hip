// The kernels of the sparse box path (include/ydbl.h: the deferred candidate sink of
// ydbl_dsconv_desc, the tile mask and candidate sink of ydbl_bottleneck_desc), in a translation unit -- and so a device
// code object -- of their own: the code objects every other session loads and runs (bneck, dsconv, dsc_lean) stay
// what they were without the path.
//   * the class tail with the sink's deferred mode: the chunked kernel (dsconv_kernel.hpp compiled with YDBL_DS_DEFER)
//     and the one-round-trip 64 -> 64 tile (dsc_lean.hpp, DEFER);
//   * the counter-zeroing kernel that also zeroes the tile masks;
//   * the masked Detect box launch that decodes the candidates' boxes (bneck_kernel.hpp compiled with
//     YDBL_BNECK_SPARSE).
#define YDBL_DS_DEFER
#define YDBL_BNECK_SPARSE
#include "bneck_kernel.hpp"
#include "dsc_lean.hpp"
#include "dsconv_kernel.hpp"

namespace ydbl {

template <int TH, int CSEG, bool DBUF>
static void ds_defer_go(const ConvArgs<_Float16>& a, const float* dww, const float* dwb, int dw_act, hipStream_t s) {
  const int tiles_x = (int)cdiv(a.Wo, 8), tiles_y = (int)cdiv(a.Ho, TH);
  const int64_t ntiles = (int64_t)a.N * tiles_y * tiles_x;
  dsconv_defer_kernel<_Float16, 3, 1, 1, TH, 8, CSEG, 4, DBUF, true><<<(unsigned)ntiles, 256, 0, s>>>(
      a, dww, dwb, dw_act, tiles_x, tiles_y, 1);  // 64 outputs: one channel split
}

bool ds_defer_tile(const ConvArgs<_Float16>& a, const float* dww, const float* dwb, int dw_act, int th, int cseg,
                   bool dbuf, hipStream_t s) {
  if (!a.sk_deferred() || a.Cout != 64) return false;
  if (th == 8 && cseg == 2 && !dbuf) return ds_defer_go<8, 2, false>(a, dww, dwb, dw_act, s), true;
  if (th == 16 && cseg == 4 && !dbuf) return ds_defer_go<16, 4, false>(a, dww, dwb, dw_act, s), true;
  if (th == 8 && cseg == 2 && dbuf) return ds_defer_go<8, 2, true>(a, dww, dwb, dw_act, s), true;
  return false;
}

__global__ __launch_bounds__(256, 1) void dsc_lean_defer_kernel(ConvArgs<_Float16> p, const float* __restrict__ dww,
                                                                 const float* __restrict__ dwb, int dw_act, int tiles_x,
                                                                 int tiles_y, int ntiles) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[LeanLds<64, 64, 3, 1, 8, 8, 256, true>::BYTES];
  lean_tile<64, 64, 3, 1, 8, 8, 256, true, true>(p, dww, dwb, dw_act, xcd_remap(blockIdx.x, ntiles), tiles_x, tiles_y,
                                                 smem);
}

void lean_defer_tile(const ConvArgs<_Float16>& a, const float* dww, const float* dwb, int dw_act, hipStream_t s) {
  const int tiles_x = (int)cdiv(a.Wo, 8), tiles_y = (int)cdiv(a.Ho, 8);
  const int ntiles = a.N * tiles_y * tiles_x;
  dsc_lean_defer_kernel<<<(unsigned)ntiles, 256, 0, s>>>(a, dww, dwb, dw_act, tiles_x, tiles_y, ntiles);
}

__global__ void ds_zero_counts_masks_kernel(int* c, int n, unsigned char* m, int nm) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) c[i] = 0;
  for (int i = threadIdx.x; i < nm; i += blockDim.x) m[i] = 0;
}

void ds_zero_counts_masks(int* counts, int n, unsigned char* masks, int nbytes, hipStream_t s) {
  ds_zero_counts_masks_kernel<<<1, 256, 0, s>>>(counts, n, masks, nbytes);
}

// The sparse Detect box launch: the same grid as the unmasked one, one workgroup per 8 x 16 tile.
template <int CIN>
static int box_sparse_go(const ydbl_bottleneck_desc* d, hipStream_t s) {
  using Cfg = BneckCfg<64, 64, 8, CIN>;
  const int tiles_x = (int)cdiv(d->y.w, Cfg::TW), tiles_y = (int)cdiv(d->y.h, 8);
  const int64_t nt = (int64_t)tiles_x * tiles_y * d->y.n;
  if (nt > 0x7fffffff) return fail(YDBL_EINVAL, "bottleneck: grid too large");
  const BoxSink sk{d->tile_mask, d->cand_box, d->cand_idx, d->cand_count, d->cand_cap, d->anchor0, d->nc,
                   d->multi_label, d->level_stride};
  bneck_sparse_kernel<64, 64, 8, false, true, CIN><<<(unsigned)nt, 256, 0, s>>>(
      dview<const _Float16>(d->x), dview<_Float16>(d->y), reinterpret_cast<const unsigned char*>(d->params), tiles_x,
      tiles_y, (int)nt, sk);
  return check_launch("ydbl_bottleneck_nhwc");
}

int box_sparse_launch(const ydbl_bottleneck_desc* d, hipStream_t s) {
  return d->x.c == 128 ? box_sparse_go<128>(d, s) : box_sparse_go<64>(d, s);
}

}  // namespace ydbl
