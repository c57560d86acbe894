// The lean DSConv tile (dsc_lean.hip) as a device function.  See dsc_lean.hip for the design.
#pragma once
#include "conv_common.hpp"

namespace ydbl {

__device__ __forceinline__ int lean_bswz(int row, int kv) { return row * 4 + (kv ^ (((row >> 2) & 1) << 1)); }

// LDS carve-up of one lean tile
template <int C, int CO, int K, int S, int TH, int TW, int NT, bool TAIL = false>
struct LeanLds {
  static constexpr int IH = (TH - 1) * S + K, IW = (TW - 1) * S + K, IWP = IW | 1, NQ = C / 4;
  static constexpr int NPX = TH * TW, NKS = C / 32;
  static constexpr int X = 0;                                              // h4 [IH * IWP * NQ]
  static constexpr int W = (X + IH * IWP * NQ * 8 + 15) / 16 * 16;          // f32x4 [K * K * NQ]
  static constexpr int B = W + K * K * NQ * 16;                             // h8 [NKS * NPX * 4]
  static constexpr int T = B + NKS * NPX * 4 * 16;                          // f32 [4][CO] class-conv weights (TAIL)
  static constexpr int BI = T + (TAIL ? 4 * CO * 4 : 0);                    // f32 [CO] pointwise bias
  static constexpr int BYTES = BI + CO * 4;
};

// One TH x TW output tile (linear tile index `tile`: image-major, then tile row, tile column).
// smem: LeanLds::BYTES of LDS, 16-byte aligned.
// DEFER (TAIL only): the tail's candidate sink in its deferred mode (conv_common.hpp, SINK_DEFER), for the kernel
// instance of the sparse box path.
template <int C, int CO, int K, int S, int TH, int TW, int NT, bool TAIL, bool DEFER = false>
__device__ __forceinline__ void lean_tile(const ConvArgs<_Float16>& p, const float* __restrict__ dww,
                                          const float* __restrict__ dwb, int dw_act, int tile, int tiles_x,
                                          int tiles_y, unsigned char* smem) {
  using T = _Float16;
  constexpr int WAVES = NT / 64;
  constexpr int CV = C / 8;                          // 16-byte vectors per pixel
  constexpr int NQ = C / 4;                          // channel quads
  constexpr int IH = (TH - 1) * S + K, IW = (TW - 1) * S + K;
  constexpr int IWP = IW | 1;                        // odd pixel pitch: rows r, r+1 in opposite bank halves
  constexpr int HV = IH * IW * CV;
  constexpr int HIT = (HV + NT - 1) / NT;
  constexpr int CSEG = NQ * TH * TW / NT;            // outputs per depthwise task
  static_assert(CSEG >= 1 && TW % CSEG == 0 && NQ * TH * (TW / CSEG) == NT, "depthwise task split");
  constexpr int SEGW = (CSEG - 1) * S + K;
  constexpr int TAPV = K * K * NQ;
  constexpr int TIT = (TAPV + NT - 1) / NT;
  constexpr int NPX = TH * TW, NTP = NPX / 16;       // 16-pixel MFMA tiles
  static_assert(NPX % 16 == 0, "tile");
  constexpr int NKS = C / 32;                        // pointwise k-steps
  constexpr int NTC = CO / 16;                       // output-channel tiles
  // per wave: a group of TN output-channel tiles (<= 64 channels; fewer for deep inputs, whose A fragments
  // [TN][NKS] would not fit the VGPRs); all 64 when CO = 64 and C <= 128 (the Detect class-conv tail needs them)
  constexpr int TNA = 16 / NKS < 1 ? 1 : 16 / NKS;
  constexpr int TN0 = NTC < (TNA < 4 ? TNA : 4) ? NTC : (TNA < 4 ? TNA : 4);
  // 64 -> 64 without the tail: a wave owns ONE 16-channel tile over all four pixel tiles instead of all 64 channels
  // of one pixel tile.  A quarter of the pointwise matrix per wave (8 KB per workgroup from L2 instead of 32 KB,
  // 8 VGPRs of A fragments instead of 32) for six more ds_read_b128 of the B tile; same MFMA chain per output.
  // bs16 at 40^2 in graph: k3 6.40 -> 5.62 us, k7 9.94 -> 9.08 us (profiles/r10/r10_partC_ab.txt).
  constexpr int TN = (C == 64 && CO == 64 && !TAIL) ? 1 : TN0;
  constexpr int NCG = NTC / TN;
  static_assert(NTC % TN == 0 && WAVES % NCG == 0, "channel groups over waves");
  constexpr int WPG = WAVES / NCG;
  constexpr int TM = (NTP + WPG - 1) / WPG;          // pixel tiles per wave
  // the activation / residual forms compiled beside the runtime one (common.hpp, with_act): the 64-channel tiles
  // only.  On the 512-thread tiles they cost 10-20 VGPRs, and 52 bytes of scratch at 256 input channels.
  constexpr bool FORMS = C <= 64;
  using L = LeanLds<C, CO, K, S, TH, TW, NT, TAIL>;
  h4* s_x = reinterpret_cast<h4*>(smem + L::X);      // fp16 halo, [row][col][quad]
  f32x4* s_w = reinterpret_cast<f32x4*>(smem + L::W);  // fp32 taps (rounded to fp16), [tap][quad]
  h8* s_b = reinterpret_cast<h8*>(smem + L::B);      // pointwise B tile, [k-step][pixel][slot]
  // activation accessors (element offsets from each view's base)
  auto ld16 = [&](const T* base, int64_t off, bool ok) -> h8 { return vload_sel(base + off, base, ok); };
  auto ld8 = [&](const T* base, int64_t off) -> h4 { return *reinterpret_cast<const h4*>(base + off); };
  auto st8 = [&](T* base, int64_t off, const float* v) { store_f<4>(base + off, v); };

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, r16 = lane & 15;
  const int cg = wave % NCG, wp = wave / NCG;
  int co[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) co[i] = (cg * TN + i) * 16 + 4 * g;  // this lane's 4 epilogue channels

  struct Tile {
    int b, oy0, ox0, iy0, ix0;
  };
  auto tile_of = [&](int t) {
    int bid = t;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    Tile tl;
    tl.b = bid / tiles_y;
    tl.oy0 = ty * TH;
    tl.ox0 = tx * TW;
    tl.iy0 = tl.oy0 * S - p.PAD;
    tl.ix0 = tl.ox0 * S - p.PAD;
    return tl;
  };
  h8 xr[HIT];
  auto load_halo = [&](const Tile& tl) {
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
      const int i = min(tid + it * NT, HV - 1);
      const int cv = i % CV, px = i / CV;
      const int hy = px / IW, hx = px - hy * IW;
      const int iy = tl.iy0 + hy, ix = tl.ix0 + hx;
      const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      xr[it] = ld16(p.x, ((int64_t)(tl.b * p.H + iy) * p.W + ix) * p.xcs + cv * 8, ok);
    }
  };

  // ---- 1. one round trip: halo + taps (-> LDS), then A fragments (+ residual) (-> VGPRs)
  const Tile tl = tile_of(tile);
  load_halo(tl);
  f32x4 wr[TIT];
#pragma unroll
  for (int it = 0; it < TIT; ++it) {
    const int i = min(tid + it * NT, TAPV - 1);
    const f32x4 w = *reinterpret_cast<const f32x4*>(dww + (i / NQ) * C + (i % NQ) * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) wr[it][e] = float(T(w[e]));  // the reference's .half() weights
  }
  // the pointwise bias (+ TAIL's class-conv weights [k][CO]) for LDS: loaded here, in the first round trip,
  // and stored just before its barrier (a store right after its load waits on every load issued before it).
  // Read from global after the MFMAs they cost one more round trip at the very end; kept in VGPRs from the start
  // they cost 16 registers and a wave per SIMD.
  constexpr int BIT = (CO + NT - 1) / NT, TLT = TAIL ? (4 * CO + NT - 1) / NT : 0;
  float bir[BIT], tlr[TLT > 0 ? TLT : 1];
#pragma unroll
  for (int it = 0; it < BIT; ++it) bir[it] = p.bias[min(tid + it * NT, CO - 1)];
#pragma unroll
  for (int it = 0; it < TLT; ++it) {
    const int i = min(tid + it * NT, 4 * CO - 1);
    tlr[it] = i / CO < p.nt3 ? p.t3w[i] : 0.f;
  }
  h8 af[TN][NKS];
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    const int row = (cg * TN + i) * 16 + r16;  // A rows: output channel of this lane
#pragma unroll
    for (int m = 0; m < NKS; ++m) af[i][m] = vload(p.w + (int64_t)row * p.KPAD + m * 32 + g * 8);
  }
#pragma unroll
  for (int it = 0; it < TIT; ++it)
    if (tid + it * NT < TAPV) s_w[tid + it * NT] = wr[it];
  {
    int64_t pp[TM];
    bool pv[TM];
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int pt = wp + WPG * j;
      const int op = pt * 16 + r16;
      const int oy = tl.oy0 + op / TW, ox = tl.ox0 + op % TW;
      pv[j] = pt < NTP && oy < p.Ho && ox < p.Wo;
      pp[j] = pv[j] ? ((int64_t)tl.b * p.Ho + oy) * p.Wo + ox : 0;
    }
    h4 rv[TN][TM];
    if (p.res != YDBL_RES_NONE) {
#pragma unroll
      for (int j = 0; j < TM; ++j)
#pragma unroll
        for (int i = 0; i < TN; ++i) rv[i][j] = ld8(p.r, pp[j] * p.rcs + co[i]);
    }
#pragma unroll
    for (int it = 0; it < HIT; ++it) {
      const int i = tid + it * NT;
      if (i < HV) {
        const int cv = i % CV, px = i / CV;
        const int hy = px / IW, hx = px - hy * IW;
        *reinterpret_cast<h8*>(&s_x[(hy * IWP + hx) * NQ + cv * 2]) = xr[it];
      }
    }
#pragma unroll
    for (int it = 0; it < BIT; ++it)
      if (tid + it * NT < CO) reinterpret_cast<float*>(smem + L::BI)[tid + it * NT] = bir[it];
#pragma unroll
    for (int it = 0; it < TLT; ++it)
      if (tid + it * NT < 4 * CO) reinterpret_cast<float*>(smem + L::T)[tid + it * NT] = tlr[it];
    __syncthreads();

    // ---- 2. depthwise: task = (quad q, output row r, segment sg), quad fastest
    {
      const int q = tid % NQ;
      const int r = (tid / NQ) % TH;
      const int sg = tid / (NQ * TH);
      float a[CSEG][4];
      constexpr int KU = K <= 3 ? K : 1;  // the 7x7: one input row's window + taps live at a time
      if constexpr (C <= 64) {
        // Window, taps and accumulators as explicit channel pairs (e0,e1), (e2,e3): one v_pk_fma_f32 per pair with
        // its operands already in adjacent registers.  Written as scalar fmaf over [4] (below), the SLP vectoriser
        // also packs, but across the quad's natural pairs, and pays a quarter of the loop's VALU issue in v_mov_b32
        // to build them.  Each lane of a packed fma is the same IEEE fma: the (ky, kx) chain per channel is unchanged.
        f32x2 a2[CSEG][2];
#pragma unroll
        for (int c = 0; c < CSEG; ++c) a2[c][0] = a2[c][1] = f32x2{0.f, 0.f};
#pragma unroll KU
        for (int ky = 0; ky < K; ++ky) {
          const h4* xrow = &s_x[((r * S + ky) * IWP + sg * CSEG * S) * NQ + q];
          f32x2 xs[SEGW][2];
#pragma unroll
          for (int i = 0; i < SEGW; ++i) {
            const h4 v = xrow[i * NQ];
            xs[i][0] = f32x2{float(v[0]), float(v[1])};
            xs[i][1] = f32x2{float(v[2]), float(v[3])};
          }
          f32x2 wv[K][2];
#pragma unroll
          for (int kx = 0; kx < K; ++kx) {
            const f32x4 w = s_w[(ky * K + kx) * NQ + q];
            wv[kx][0] = w.lo;
            wv[kx][1] = w.hi;
          }
#pragma unroll
          for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int c = 0; c < CSEG; ++c)
#pragma unroll
              for (int h = 0; h < 2; ++h) a2[c][h] = __builtin_elementwise_fma(xs[c * S + kx][h], wv[kx][h], a2[c][h]);
        }
#pragma unroll
        for (int c = 0; c < CSEG; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) a[c][e] = a2[c][e >> 1][e & 1];
      } else {
        // the 512-thread tiles keep the scalar form: with pairs they take fewer registers (k3 188 -> 138, stride 2
        // 170 -> 123) and more waves per SIMD, and DBL-s bs8, which runs them at 40^2, lost 0.5 % (profiles/r10/)
#pragma unroll
        for (int c = 0; c < CSEG; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) a[c][e] = 0.f;
#pragma unroll KU
        for (int ky = 0; ky < K; ++ky) {
          const h4* xrow = &s_x[((r * S + ky) * IWP + sg * CSEG * S) * NQ + q];
          float xs[SEGW][4];
#pragma unroll
          for (int i = 0; i < SEGW; ++i) {
            const h4 v = xrow[i * NQ];
#pragma unroll
            for (int e = 0; e < 4; ++e) xs[i][e] = float(v[e]);
          }
          f32x4 wv[K];
#pragma unroll
          for (int kx = 0; kx < K; ++kx) wv[kx] = s_w[(ky * K + kx) * NQ + q];
#pragma unroll
          for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int c = 0; c < CSEG; ++c)
#pragma unroll
              for (int e = 0; e < 4; ++e) a[c][e] = fmaf(xs[c * S + kx][e], wv[kx][e], a[c][e]);
        }
      }
      if (dwb) {  // uniform: DWConv (+ folded BN) bias and activation before the pointwise
        const f32x4 bq = *reinterpret_cast<const f32x4*>(dwb + q * 4);
        with_act<T>(dw_act, !FORMS || p.epi_generic, [&](auto A) {  // resolved once, not per value (common.hpp)
#pragma unroll
          for (int c = 0; c < CSEG; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) a[c][e] = act_as<T, decltype(A)::value>(a[c][e] + bq[e], dw_act);
        });
      }
      const int ks = q / 8, ql = q % 8;  // k-step and 4-channel slot of this quad
#pragma unroll
      for (int c = 0; c < CSEG; ++c) {
        const int px = r * TW + sg * CSEG + c;
        *(reinterpret_cast<h4*>(&s_b[ks * NPX * 4 + lean_bswz(px, ql >> 1)]) + (ql & 1)) = to_h4_rne(a[c]);
      }
    }
    __syncthreads();

    // ---- 3. pointwise MFMA over all k-steps, epilogue
    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < NKS; ++m)
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int pt = wp + WPG * j;
        if (TM * WPG == NTP || pt < NTP) {
          const h8 bf = s_b[m * NPX * 4 + lean_bswz(pt * 16 + r16, g)];
#pragma unroll
          for (int i = 0; i < TN; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][m], bf, acc[i][j], 0, 0, 0);
        }
      }
    float bv[TN][4];
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(smem + L::BI + co[i] * 4);
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[i][q] = b4[q];
    }
    float ys[TAIL ? TN : 1][TAIL ? TM : 1][4];  // TAIL: the stored y values for the class conv
    // the epilogue for activation A and residual mode R (codes, or ACT_RT / -1: p.act / p.res at run time)
    auto epilogue = [&](auto A, auto R) {
      constexpr int AC = decltype(A)::value, RC = decltype(R)::value;
      const int res = RC < 0 ? p.res : RC;
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        if (!pv[j]) continue;
#pragma unroll
        for (int i = 0; i < TN; ++i) {
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = act_as<T, AC>(acc[i][j][q] + bv[i][q], p.act);
          if (res == YDBL_RES_ADD) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = AC == ACT_RT ? float(rv[i][j][q]) + v[q] : add_rn(float(rv[i][j][q]), v[q]);
          } else if (res == YDBL_RES_MUL) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = float(rv[i][j][q]) * v[q];
          }
          if (!(TAIL && p.y_off)) st8(p.y, pp[j] * p.ycs + co[i], v);  // (uniform) the tail's y may have no reader
          if constexpr (TAIL) {
#pragma unroll
            for (int q = 0; q < 4; ++q) ys[i][j][q] = round_to<T>(v[q]);
          }
        }
      }
    };
    // decided once per wave: SiLU / none with residual none / add run straight-line code, the rest the runtime form
    const bool lean = FORMS && !p.epi_generic && p.res != YDBL_RES_MUL;
    if (lean && p.act == YDBL_ACT_SILU) {
      if (p.res == YDBL_RES_ADD) epilogue(ActC<YDBL_ACT_SILU>{}, ActC<YDBL_RES_ADD>{});
      else epilogue(ActC<YDBL_ACT_SILU>{}, ActC<YDBL_RES_NONE>{});
    } else if (lean && p.act == YDBL_ACT_NONE) {
      if (p.res == YDBL_RES_ADD) epilogue(ActC<YDBL_ACT_NONE>{}, ActC<YDBL_RES_ADD>{});
      else epilogue(ActC<YDBL_ACT_NONE>{}, ActC<YDBL_RES_NONE>{});
    } else {
      epilogue(ActC<ACT_RT>{}, ActC<-1>{});
    }
    if constexpr (TAIL && NCG == 1 && TN == 4) {  // Detect class conv over the 64 output channels (CO == 64)
      conv_tail_1x1_vals<T, TN, TM, DEFER ? SINK_DEFER : SINK_BOX>(p, ys, pp, pv, co, g,
                                                                   reinterpret_cast<const float*>(smem + L::T));
    }
  }
}

}  // namespace ydbl
