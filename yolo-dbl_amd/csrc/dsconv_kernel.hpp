// The chunked DSConv kernel of dsconv.hip (design notes there), in a header because two translation units compile it:
//   dsconv.hip        dsconv_kernel -- every DSConv / DWConv -> Conv1x1 launch, with SINK the box-reading candidate sink;
//   sparse_box.hip    with YDBL_DS_DEFER defined: dsconv_defer_kernel, whose SINK instances run the sink's deferred mode.
// The preprocessor, not a template parameter, picks the mode, so dsconv_kernel keeps its name, its arguments and its code
// object, and the deferred instances live in a code object of their own.
#pragma once
#include "conv_common.hpp"

#ifdef YDBL_DS_DEFER
#define YDBL_DSCONV_KERNEL dsconv_defer_kernel
#define YDBL_DS_SINK_MODE SINK_DEFER
#else
#define YDBL_DSCONV_KERNEL dsconv_kernel
#define YDBL_DS_SINK_MODE SINK_BOX
#endif

namespace ydbl {

template <int R>
__device__ __forceinline__ int bswz(int row, int kv) {  // B-tile slot: 16 consecutive rows -> distinct banks
  return row * 4 + (kv ^ (((row >> 2) & 1) << 1));
}

// 4 consecutive activation-dtype channels from 4 fp32 values (8 B f16 / 16 B f32).
__device__ __forceinline__ void store4(_Float16* d, const float* a) { *reinterpret_cast<h4*>(d) = to_h4_rne(a); }
__device__ __forceinline__ void store4(float* d, const float* a) {
  *reinterpret_cast<f32x4*>(d) = f32x4{a[0], a[1], a[2], a[3]};
}

// SINK: the class-conv tail also emits the NMS candidates (conv_common.hpp, tail_store): an instance of its own,
// built for the Detect pair's shape only (fp16, k3 s1, 64 outputs), so that every other launch runs the plain code.
template <typename T, int K, int S, int DIL, int TH, int TW, int CSEG, int NTN, bool DBUF, bool SINK = false>
__global__ __launch_bounds__(256, 2) void YDBL_DSCONV_KERNEL(ConvArgs<T> p, const float* __restrict__ dww,
                                                             const float* __restrict__ dwb, int dw_act, int tiles_x,
                                                             int tiles_y, int co_splits) {
  constexpr int VEC = Vec<T>::N;
  constexpr int CC = 4 * VEC;    // channels per chunk (one pointwise MFMA k-step)
  constexpr int NQ = CC / 4;     // fp32 quads per staged pixel
  constexpr int QV = VEC / 4;    // quads per 16-byte activation vector
  constexpr int IH = (TH - 1) * S + (K - 1) * DIL + 1, IW = (TW - 1) * S + (K - 1) * DIL + 1;
  constexpr int IWP = IW | 1;    // odd row pitch: the rows of a half-wave hit distinct bank quarters
  constexpr int NSEG = TW / CSEG;
  static_assert(TW % CSEG == 0, "segments");
  constexpr int NTASK = NQ * TH * NSEG;  // (quad, row, segment), quad fastest
  constexpr int SEGW = (CSEG - 1) * S + (K - 1) * DIL + 1;
  constexpr int HALO = IH * IW * 4;      // 16-byte activation vectors to stage per chunk
  constexpr int HIT = (HALO + 255) / 256;
  constexpr int NT = TH * TW / 16;       // 16-pixel MFMA tiles
  static_assert(TH * TW % 16 == 0, "tile");
  constexpr int TMW = (NT + 3) / 4;
  using vec = typename Vec<T>::type;
  // the halo and the taps are staged as fp32 (converted once per element, not once per tap use)
  constexpr int NB = DBUF ? 2 : 1;  // double-buffered halo, or one buffer refilled between barriers
  __shared__ f32x4 s_x[NB][IH * IWP * NQ];
  __shared__ f32x4 s_w[NB][K * K * NQ];
  __shared__ vec s_b[TH * TW * 4];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, r16 = lane & 15;
  const int ntiles = p.N * tiles_y * tiles_x;
  int bid = xcd_remap(blockIdx.x, ntiles * co_splits);
  const int cs = bid % co_splits;
  bid /= co_splits;
  const int tx = bid % tiles_x; bid /= tiles_x;
  const int ty = bid % tiles_y;
  const int b = bid / tiles_y;
  const int oy0 = ty * TH, ox0 = tx * TW;
  const int iy0 = oy0 * S - p.PAD, ix0 = ox0 * S - p.PAD;
  const int co0 = cs * NTN * 16;
  __shared__ __align__(16) float s_bias[NTN * 16];
  BiasStage<NTN * 16> bst;
  bst.fetch(p.bias, co0, p.Cout);

  constexpr int TAPV = K * K * NQ;  // fp32 tap quads per chunk (392 for k7 f16: > one per thread)
  constexpr int TIT = (TAPV + 255) / 256;
  // raw loads now, zero selects / tap rounding at the LDS store: the next chunk's loads stay in flight through
  // this chunk's depthwise and pointwise phases (a select or conversion next to its load waits for it there)
  vec xr[HIT];
  bool xok[HIT];
  f32x4 wr[TIT];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
      const int i = min(tid + it * 256, HALO - 1);
      const int cv = i & 3, px = i >> 2;
      const int hy = px / IW, hx = px - hy * IW;
      const int iy = iy0 + hy, ix = ix0 + hx;
      xok[it] = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      xr[it] = vload_clamped(p.x + ((int64_t)(b * p.H + iy) * p.W + ix) * p.xcs + c0 + cv * VEC, p.x, xok[it]);
    }
#pragma unroll
    for (int it = 0; it < TIT; ++it) {
      const int i = min(tid + it * 256, TAPV - 1);
      const int tap = i / NQ, q = i % NQ;
      wr[it] = *reinterpret_cast<const f32x4*>(dww + tap * p.Cin + c0 + q * 4);
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
      const int i = tid + it * 256;
      if (i < HALO) {
        const int cv = i & 3, px = i >> 2;
        const int hy = px / IW, hx = px - hy * IW;
        f32x4* d = &s_x[buf][(hy * IWP + hx) * NQ + cv * QV];
        const vec xv = vsel(xr[it], xok[it]);
#pragma unroll
        for (int u = 0; u < QV; ++u)
          d[u] = f32x4{float(xv[4 * u]), float(xv[4 * u + 1]), float(xv[4 * u + 2]), float(xv[4 * u + 3])};
      }
    }
#pragma unroll
    for (int it = 0; it < TIT; ++it)  // taps rounded to the activation dtype (the reference's .half() weights)
      if (tid + it * 256 < TAPV)
        s_w[buf][tid + it * 256] = f32x4{float(T(wr[it][0])), float(T(wr[it][1])), float(T(wr[it][2])), float(T(wr[it][3]))};
  };

  f32x4 acc[NTN][TMW];
#pragma unroll
  for (int i = 0; i < NTN; ++i)
#pragma unroll
    for (int j = 0; j < TMW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = p.Cin / CC;
  load_chunk(0);
  store_chunk(0);
  bst.commit(s_bias);
  __syncthreads();
  for (int ch = 0; ch < nchunks; ++ch) {
    const int buf = DBUF ? (ch & 1) : 0;
    const int c0 = ch * CC;
    // this chunk's pointwise A fragments first (loads complete in order: waiting for them later does not wait
    // for the next chunk's), zero rows past Cout selected at the MFMAs
    vec af[NTN];
#pragma unroll
    for (int i = 0; i < NTN; ++i) {
      const int co = co0 + i * 16 + r16;
      af[i] = vload_clamped(p.w + (int64_t)co * p.KPAD + c0 + g * VEC, p.w, co < p.Cout);
    }
    if (ch + 1 < nchunks) load_chunk(c0 + CC);
    // ---- depthwise phase
    for (int task = tid; task < NTASK; task += 256) {
      const int q = task % NQ;
      const int r = (task / NQ) % TH;
      const int sg = task / (NQ * TH);
      float a[CSEG][4];
#pragma unroll
      for (int c = 0; c < CSEG; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) a[c][e] = 0.f;
#pragma unroll 1
      for (int ky = 0; ky < K; ++ky) {  // rolled: one input row's window + taps live at a time
        const f32x4* xrow = &s_x[buf][((r * S + ky * DIL) * IWP + sg * CSEG * S) * NQ + q];
        f32x4 xs[SEGW], wv[K];
#pragma unroll
        for (int i = 0; i < SEGW; ++i) xs[i] = xrow[i * NQ];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) wv[kx] = s_w[buf][(ky * K + kx) * NQ + q];
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
          for (int c = 0; c < CSEG; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) a[c][e] = fmaf(xs[c * S + kx * DIL][e], wv[kx][e], a[c][e]);
      }
      if (dwb) {  // uniform: DWConv (+ folded BN) bias and activation before the pointwise
        const f32x4 bq = *reinterpret_cast<const f32x4*>(dwb + c0 + q * 4);
#pragma unroll
        for (int c = 0; c < CSEG; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) a[c][e] = apply_act<T>(a[c][e] + bq[e], dw_act);
      }
#pragma unroll
      for (int c = 0; c < CSEG; ++c) {
        const int px = r * TW + sg * CSEG + c;
        store4(reinterpret_cast<T*>(&s_b[bswz<0>(px, q / QV)]) + (q % QV) * 4, a[c]);
      }
    }
    __syncthreads();
    // ---- pointwise phase
#pragma unroll
    for (int j = 0; j < TMW; ++j) {
      const int t = wave + 4 * j;
      if (t < NT) {
        const vec bf = s_b[bswz<0>(t * 16 + r16, g)];
#pragma unroll
        for (int i = 0; i < NTN; ++i) acc[i][j] = mfma_chunk<T>(vsel(af[i], co0 + i * 16 + r16 < p.Cout), bf, acc[i][j]);
      }
    }
    if constexpr (DBUF) {
      if (ch + 1 < nchunks) store_chunk(buf ^ 1);
    } else {
      if (ch + 1 < nchunks) {
        __syncthreads();  // every wave is past this chunk's depthwise reads
        store_chunk(0);
      }
    }
    __syncthreads();
  }

  int64_t pp[TMW];
  bool pv[TMW];
#pragma unroll
  for (int j = 0; j < TMW; ++j) {
    const int t = wave + 4 * j;
    const int op = t * 16 + r16;
    const int oy = oy0 + op / TW, ox = ox0 + op % TW;
    pv[j] = t < NT && oy < p.Ho && ox < p.Wo;
    pp[j] = ((int64_t)b * p.Ho + oy) * p.Wo + ox;
  }
  int co[NTN];
#pragma unroll
  for (int i = 0; i < NTN; ++i) co[i] = co0 + i * 16 + 4 * g;
  // the runtime-dispatch form only: a compiled SiLU / none form beside it (conv_common.hpp) cost this kernel 4-24
  // VGPRs, a wave per SIMD on the k5 / k7 tiles and 20 bytes of scratch on the stride-2 ones
  conv_epilogue<T, NTN, TMW, false, ACT_RT>(p, acc, pp, pv, co, s_bias, co0);
  if constexpr (NTN == 4) {  // the tail is only launched with Cout 64 = NTN * 16 (host-checked)
    if (p.t3w) conv_tail_1x1<T, NTN, TMW, SINK ? YDBL_DS_SINK_MODE : SINK_NONE>(p, acc, pp, pv, co, g);
  }
}

}  // namespace ydbl
