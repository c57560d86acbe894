// DSConv fused into one kernel (U/nn/modules/conv.py:91-108: SiLU(BN(pw1x1(dw_kxk(x))))), BN
// folded into the pointwise weights.  The depthwise output never touches HBM.
//
// A workgroup owns a TH x TW output tile and NTN*16 output channels.  For each chunk of
// CC = 4*VEC input channels (= one MFMA k-step of the pointwise):
//   1. the chunk's input halo tile and depthwise taps sit in LDS as fp32 (converted once per
//      element at staging; the next chunk's halo is loaded into registers before this chunk's
//      arithmetic and stored after it, into a second buffer or the refilled single one),
//   2. depthwise phase: a thread owns CSEG consecutive outputs of one row and one fp32 quad of
//      channels; it slides a (CSEG-1)*S + K register window along each input row, so every LDS
//      element it reads feeds up to K outputs (fp32 accumulate in the reference's (ky, kx) tap
//      order; padded taps read staged zeros, fma(0, w, a) == a), rounds to the activation dtype
//      (the reference's fp16 dw output) and writes the MFMA B tile [TH*TW px][CC],
//   3. pointwise phase: wave w multiplies its 16-pixel tiles w, w+4, ... by the chunk's
//      pointwise weights (A fragments loaded from the L2-resident [Cout][KPAD] matrix at the top
//      of the chunk) into NTN x TMW 16x16 accumulators.
// Fused epilogue (bias, SiLU, residual add of DSBottleneck, channel-slice store) as conv.hip.
#include "dsconv_kernel.hpp"

namespace ydbl {

template <typename T, int K, int S, int DIL, int TH, int TW, int CSEG, bool DBUF = true>
static void launch_ds_tile(const ConvArgs<T>& a, const float* dww, const float* dwb, int dw_act, hipStream_t s) {
  const int tiles_x = (int)cdiv(a.Wo, TW), tiles_y = (int)cdiv(a.Ho, TH);
  const int64_t ntiles = (int64_t)a.N * tiles_y * tiles_x;
  auto go = [&](auto kern, int ntn) {
    const int cs = (int)cdiv(a.Cout, ntn * 16);
    kern<<<(unsigned)(ntiles * cs), 256, 0, s>>>(a, dww, dwb, dw_act, tiles_x, tiles_y, cs);
  };
  if constexpr (sizeof(T) == 2 && K == 3 && S == 1 && DIL == 1) {
    if (a.sk_deferred()) {  // the deferred sink: SINK_DEFER instances only (sparse_box.hip)
      if (TW != 8 || !ds_defer_tile(a, dww, dwb, dw_act, TH, CSEG, DBUF, s))
        fail(YDBL_EINVAL, "dsconv: no deferred-sink instance for this tile");
      return;
    }
    if (a.sk.ccount) return go(dsconv_kernel<T, K, S, DIL, TH, TW, CSEG, 4, DBUF, true>, 4);  // (Cout 64: ds_check)
  }
  if (a.sk_deferred()) {  // (ds_check admits the sink for fp16 k3 s1 only)
    fail(YDBL_EINVAL, "dsconv: the deferred sink needs fp16, k 3, stride 1");
    return;
  }
  if (a.Cout <= 32) go(dsconv_kernel<T, K, S, DIL, TH, TW, CSEG, 2, DBUF>, 2);
  // k3 s1 with < 512 tiles: two 64-channel column workgroups per tile (the cheap depthwise phase is
  // recomputed; 128->128 @20^2 bs32 15.0 -> 11.8 us; k7 loses: 19.7 -> 25.4)
  else if (a.Cout <= 64 || ntiles < 256 || (K == 3 && S == 1 && ntiles < 512))
    go(dsconv_kernel<T, K, S, DIL, TH, TW, CSEG, 4, DBUF>, 4);
  else go(dsconv_kernel<T, K, S, DIL, TH, TW, CSEG, 8, DBUF>, 8);
}

// Tile shape (measured on the DBL-n/s shapes, fp16 bs 32): maps wider than 20 px take a 16x8 tile
// with 4-output row segments and one refilled LDS buffer (small footprint: 3-4 workgroups per CU
// hide each other's halo loads; 40^2 k7 64ch 25.8 -> 15.1 us); 20-px and smaller maps take an 8x8
// double-buffered tile (more workgroups on the few pixels).
template <typename T, int K, int S, int DIL>
static int launch_ds(const ConvArgs<T>& a, const float* dww, const float* dwb, int dw_act, hipStream_t s) {
  if constexpr (sizeof(T) == 2) {
    if (try_dsc_lean(a, dww, dwb, dw_act, K, S, DIL, s)) return check_launch("ydbl_dsconv_nhwc");
  }
  // Fewer than 400 16x8 tiles (the bench's bs16 sub-batch graphs at 40^2: 240): 8x8 single-buffered
  // tiles, 1.7x the workgroups (DBL-n bs32 on two streams 13.98 k -> 14.45 k img/s; at bs32 / 480 tiles
  // the two are even, and the 16x8 tile stays ahead on DBL-s bs64 and DBL-l 1280)
  const int64_t t168 = (int64_t)a.N * cdiv(a.Ho, 16) * cdiv(a.Wo, 8);
  if (a.Wo > 20 && t168 < 400) launch_ds_tile<T, K, S, DIL, 8, 8, 2, false>(a, dww, dwb, dw_act, s);
  else if (a.Wo > 20) launch_ds_tile<T, K, S, DIL, 16, 8, 4, false>(a, dww, dwb, dw_act, s);
  else launch_ds_tile<T, K, S, DIL, 8, 8, 2, true>(a, dww, dwb, dw_act, s);
  return check_launch("ydbl_dsconv_nhwc");
}

template <typename T>
static ConvArgs<T> ds_args(const ydbl_dsconv_desc* d) {
  ConvArgs<T> a{};
  a.x = reinterpret_cast<const T*>(d->x.ptr);
  a.xcs = d->x.cs; a.N = d->x.n; a.H = d->x.h; a.W = d->x.w; a.Cin = d->x.c;
  a.y = reinterpret_cast<T*>(d->y.ptr);
  a.ycs = d->y.cs; a.Ho = d->y.h; a.Wo = d->y.w; a.Cout = d->y.c;
  a.r = reinterpret_cast<const T*>(d->r.ptr); a.rcs = d->r.cs;
  a.w = reinterpret_cast<const T*>(d->pw_w); a.bias = d->bias;
  a.KW = d->k; a.S = d->stride; a.PAD = d->pad; a.DIL = d->dil;
  a.K = d->x.c; a.KPAD = d->kpad;
  a.act = d->act; a.res = d->res_mode;
  a.epi_generic = epi_generic();
  if (d->tail_w) {
    a.t3w = d->tail_w; a.t3b = d->tail_b; a.nt3 = d->tail_n;
    a.y3 = reinterpret_cast<T*>(d->tail_y.ptr); a.y3cs = d->tail_y.cs;
    a.y_off = d->y_unused;
    if (d->cand_count) {
      a.sk = CandSink{d->cand_box, d->cand_score, d->cand_cls, d->cand_idx, d->cand_count, d->cand_cap,
                      d->conf_thres, d->multi_label, d->classes, d->nclasses};
      a.skbox = reinterpret_cast<const T*>(d->box.ptr); a.skboxcs = d->box.cs;
      a.ska0 = d->anchor0; a.skstride = d->level_stride;
      if (d->tile_mask) a.sk_defer(d->tile_mask, d->mask_tiles_x);  // no cand_box, the box fields carry the tile mask
    }
  }
  a.P = d->y.n * d->y.h * d->y.w;
  return a;
}

ConvArgs<_Float16> ds_args_f16(const ydbl_dsconv_desc* d) { return ds_args<_Float16>(d); }

template <typename T>
static int run_ds(const ydbl_dsconv_desc* d, hipStream_t s) {
  const ConvArgs<T> a = ds_args<T>(d);
  if (d->k == 3 && d->stride == 1 && d->dil == 1) return launch_ds<T, 3, 1, 1>(a, d->dw_w, d->dw_bias, d->dw_act, s);
  if (d->k == 3 && d->stride == 2 && d->dil == 1) return launch_ds<T, 3, 2, 1>(a, d->dw_w, d->dw_bias, d->dw_act, s);
  if (d->k == 5 && d->stride == 1 && d->dil == 1) return launch_ds<T, 5, 1, 1>(a, d->dw_w, d->dw_bias, d->dw_act, s);
  if (d->k == 7 && d->stride == 1 && d->dil == 1) return launch_ds<T, 7, 1, 1>(a, d->dw_w, d->dw_bias, d->dw_act, s);
  return fail(YDBL_EINVAL, "dsconv: supported (k, stride, dil): (3,1,1) (3,2,1) (5,1,1) (7,1,1)");
}

// The descriptor rules of ydbl_dsconv_nhwc (include/ydbl.h).
int ds_check(const ydbl_dsconv_desc* d) {
  if (!d) return fail(YDBL_EINVAL, "dsconv: null descriptor");
  if (check_view(&d->x, "dsconv.x", true) || check_view(&d->y, "dsconv.y", false)) return YDBL_EINVAL;
  if (d->x.dtype != d->y.dtype || d->x.n != d->y.n) return fail(YDBL_EINVAL, "dsconv: x/y mismatch");
  const int cc = d->x.dtype == YDBL_F16 ? 32 : 16;
  if (d->x.c % cc) return fail(YDBL_EINVAL, "dsconv: Cin must be a multiple of 32 (f16) / 16 (f32)");
  const int ho = (d->x.h + 2 * d->pad - d->dil * (d->k - 1) - 1) / d->stride + 1;
  const int wo = (d->x.w + 2 * d->pad - d->dil * (d->k - 1) - 1) / d->stride + 1;
  if (ho != d->y.h || wo != d->y.w) return fail(YDBL_EINVAL, "dsconv: output spatial size mismatch");
  if (!d->dw_w || !d->pw_w) return fail(YDBL_EINVAL, "dsconv: null weights");
  if (d->kpad < d->x.c || d->kpad % 32) return fail(YDBL_EINVAL, "dsconv: kpad must be >= Cin and a multiple of 32");
  if (d->y.cs % 4) return fail(YDBL_EINVAL, "dsconv: output channel stride must be a multiple of 4");
  if (d->res_mode != YDBL_RES_NONE) {
    if (check_view(&d->r, "dsconv.r", false)) return YDBL_EINVAL;
    if (d->r.cs % 4 || d->r.dtype != d->y.dtype || d->r.n != d->y.n || d->r.h != d->y.h || d->r.w != d->y.w ||
        d->r.c < d->y.c)
      return fail(YDBL_EINVAL, "dsconv: residual shape mismatch");
  }
  if (d->tail_w) {
    if (!d->tail_b || d->tail_n < 1 || d->tail_n > 4 || d->y.c != 64 || d->res_mode != YDBL_RES_NONE ||
        check_view(&d->tail_y, "dsconv.tail_y", false) || d->tail_y.c != d->tail_n || d->tail_y.dtype != d->y.dtype ||
        d->tail_y.n != d->y.n || d->tail_y.h != d->y.h || d->tail_y.w != d->y.w)
      return fail(YDBL_EINVAL, "dsconv: tail needs y.c 64, 1 <= tail_n <= 4, tail_y [n,h,w,tail_n] of y's dtype, no residual");
  }
  if (d->y_unused && !d->tail_w) return fail(YDBL_EINVAL, "dsconv: y_unused needs the tail (its output is the launch's result)");
  if (d->cand_count) {
    if (!d->tail_w || d->y.dtype != YDBL_F16 || !d->cand_box || !d->cand_score || !d->cand_cls || !d->cand_idx ||
        d->cand_cap < 1 || d->anchor0 < 0 || (d->nclasses > 0 && !d->classes) || d->k != 3 || d->stride != 1 ||
        d->dil != 1)
      return fail(YDBL_EINVAL, "dsconv: the candidate sink needs the tail, fp16, k 3 / stride 1 / dil 1 (the Detect "
                               "pair) and all five candidate arrays");
    if (d->tile_mask) {  // deferred: the box view is not read
      const int64_t mtx = cdiv(d->y.w, 16), mti = mtx * cdiv(d->y.h, 8);
      if (d->mask_tiles_x != mtx || d->mask_tiles_img != mti)
        return fail(YDBL_EINVAL, "dsconv: the tile mask is 8-row x 16-column tiles: mask_tiles_x = ceil(w / 16), "
                                 "mask_tiles_img = mask_tiles_x * ceil(h / 8)");
    } else if (check_view(&d->box, "dsconv.box", true) || d->box.c != 64 || d->box.dtype != YDBL_F16 ||
               d->box.n != d->y.n || d->box.h != d->y.h || d->box.w != d->y.w) {
      return fail(YDBL_EINVAL, "dsconv: the sink's box view must be fp16 [n,h,w,64] of y's map, 16-byte aligned");
    }
    if (d->mask_zero_bytes < 0 || (d->mask_zero_bytes > 0 && !d->mask_zero))
      return fail(YDBL_EINVAL, "dsconv: mask_zero_bytes without mask_zero");
  } else if (d->tile_mask || d->mask_zero) {
    return fail(YDBL_EINVAL, "dsconv: the tile mask belongs to the candidate sink (cand_count is NULL)");
  }
  return YDBL_OK;
}

// Zeroes the candidate counters ahead of the first level's tile kernel (a kernel, not hipMemsetAsync: detect.hip,
// zero_counts_kernel, records why).  With tile masks to zero as well the call launches ds_zero_counts_masks instead.
__global__ void ds_zero_counts_kernel(int* c, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) c[i] = 0;
}

}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_dsconv_nhwc(const ydbl_dsconv_desc* d, void* stream) {
  if (const int rc = ds_check(d)) return rc;
  const hipStream_t s = as_stream(stream);
  if (d->cand_count && d->zero_counts) {
    if (d->mask_zero && d->mask_zero_bytes > 0) ds_zero_counts_masks(d->cand_count, d->y.n, d->mask_zero, d->mask_zero_bytes, s);
    else ds_zero_counts_kernel<<<1, 256, 0, s>>>(d->cand_count, d->y.n);
  }
  return d->x.dtype == YDBL_F16 ? run_ds<_Float16>(d, s) : run_ds<float>(d, s);
}
