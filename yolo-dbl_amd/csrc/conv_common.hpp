// Shared pieces of the MFMA convolution kernels (conv.hip, dsconv.hip): argument block,
// MFMA k-chunk (f16 16x16x32 / exact f32 4x 16x16x4) and the fused epilogue.
#pragma once
#include "common.hpp"
#include "decode_math.hpp"

namespace ydbl {

template <typename T>
struct ConvArgs {
  const T* x; int xcs; int N, H, W, Cin;
  T* y; int ycs; int Ho, Wo, Cout;
  const T* r; int rcs;
  const T* w; const float* bias;
  int KW, S, PAD, DIL, K, KPAD;
  int act, res;
  int P;
  T* y2; int y2cs;  // optional second output y2 = a2 * T(v) + b2 * r2 (fused FullPAD)
  const T* r2; int r2cs;
  float a2, b2;
  // fp8 operand mode (dq != nullptr): w holds OCP e4m3 bytes [Cout][KPAD] (per-output-channel
  // scale sw), activations are quantized to e4m3 with the per-tensor scale qs as they are staged,
  // and the accumulator is dequantized by dq[co] = 1 / (sw[co] * qs) before bias / activation.
  const float* dq;
  float qs;
  // optional trailing 1x1 conv of nt3 (<= 4) outputs over all Cout channels (dsconv.hip, Detect cls):
  // y3[p][k] = sum_c t3w[k][c] * T(y[p][c]) + t3b[k]
  const float* t3w; const float* t3b;
  T* y3; int y3cs; int nt3;
  // optional NMS-candidate sink of that tail (sk.ccount != nullptr; fp16, nt3 = the class count): the launch is one
  // Detect level's class branch and appends the level's candidates itself (tail_store below).  skbox: the
  // level's 64 box logits per pixel, ska0: the level's first anchor, skstride: its stride.
  // The sink's deferred mode (sk.cbox == nullptr; instances of their own, SINK_DEFER) reads no box and writes no
  // cand_box, and flags the candidates' 8 x 16 tiles instead (include/ydbl.h): there skbox is the tile mask's bytes
  // [N][ceil(Ho / 8)][skboxcs] and skboxcs the tiles per row -- no field of its own, since this block is an argument of
  // every convolution kernel and a longer one changes the code of all of them.
  CandSink sk;
  const T* skbox; int skboxcs; int ska0; float skstride;
  int y_off;  // the tail launch leaves y unwritten (nothing reads it)
  // split-K (conv_wsk_kernel): ksplit > 1 -> fp32 partial tiles ws[z][P][round_up(Cout, 4)], summed + epilogue by
  // splitk_epilogue_kernel
  float* ws; int64_t ws_bytes; int ksplit;
  int epi_generic;  // YDBL_EPI_GENERIC=1: every epilogue takes its runtime-dispatch form (common.hpp, with_act)

  // The deferred sink's view of the box fields.  Only these three functions know the double use: sk_defer() sets it
  // up, the launchers ask sk_deferred() and hand such arguments to SINK_DEFER instances only (anything else is
  // refused: launch_ds_tile, try_dsc_lean), and those instances read the mask through sk_mask().
  void sk_defer(unsigned char* mask, int tiles_x) {
    sk.cbox = nullptr;
    skbox = reinterpret_cast<const T*>(mask);
    skboxcs = tiles_x;
  }
  __host__ __device__ bool sk_deferred() const { return sk.ccount != nullptr && sk.cbox == nullptr; }
  // the mask byte of pixel (gy, gx) of image b: tiles of 8 rows x 16 columns, skboxcs per row
  __device__ __forceinline__ unsigned char* sk_mask(int b, int gy, int gx) const {
    unsigned char* m = reinterpret_cast<unsigned char*>(const_cast<T*>(skbox));
    return m + ((int64_t)b * ((Ho + 7) >> 3) + (gy >> 3)) * skboxcs + (gx >> 4);
  }
};

// the candidate sink a tail instance is compiled for
constexpr int SINK_NONE = 0, SINK_BOX = 1, SINK_DEFER = 2;

// ---- operand policy: f16/f32 vectors, or 8-byte groups of 8 e4m3 values (fp8 MFMA) -----------
template <typename T, bool Q8> struct Op {
  using lds = typename Vec<T>::type;
};
template <> struct Op<_Float16, true> {
  using lds = uint64_t;
};

// 8 activations -> 8 OCP e4m3 bytes (k order kept: byte i = element i), scaled and saturated
__device__ __forceinline__ uint64_t quant_e4m3(const h8& v, float s) {
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = fminf(fmaxf(float(v[i]) * s, -448.f), 448.f);
  int lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  int hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return (uint64_t)(uint32_t)lo | ((uint64_t)(uint32_t)hi << 32);
}

template <typename T, bool Q8>
__device__ __forceinline__ typename Op<T, Q8>::lds to_op(const typename Vec<T>::type& v, float s) {
  if constexpr (Q8) return quant_e4m3(v, s);
  else return v;
}

// weight (A operand) load of one k-vector: VEC elements of T, or 8 e4m3 bytes at the same
// element offset (the fp8 matrix is [Cout][KPAD] bytes); load_wop_raw leaves the zero select to the consumer
template <typename T, bool Q8>
__device__ __forceinline__ typename Op<T, Q8>::lds load_wop_raw(const T* w, int64_t off, bool ok) {
  if constexpr (Q8) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(w);
    return *reinterpret_cast<const uint64_t*>(b + (ok ? off : 0));
  } else {
    return vload_clamped(w + off, w, ok);
  }
}
template <typename T, bool Q8>
__device__ __forceinline__ typename Op<T, Q8>::lds load_wop(const T* w, int64_t off, bool ok) {
  if constexpr (Q8) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(w);
    const uint64_t v = *reinterpret_cast<const uint64_t*>(b + (ok ? off : 0));
    return ok ? v : 0ull;
  } else {
    return vload_sel(w + off, w, ok);
  }
}


// LDS slot of halo pixel `pix` (row-major over the halo tile), k-vector g, in the halo kernels' "planar per 16-lane
// run" layout (conv3x3.hip)
template <int S>
__device__ __forceinline__ int hslot(int pix, int g) {
  return (pix / (16 * S)) * (64 * S) + g * (16 * S) + (pix % S) * 16 + ((pix / S) & 15);
}

// dsc_lean.hip: one-round-trip DSConv / DWConv->Conv1x1 for the small-map shapes it is built for.
// dsconv.hip: a ydbl_dsconv_desc's kernel arguments (fp16) and its descriptor rules (YDBL_OK or the error code).
ConvArgs<_Float16> ds_args_f16(const ydbl_dsconv_desc* d);
int ds_check(const ydbl_dsconv_desc* d);
bool try_dsc_lean(const ConvArgs<_Float16>& a, const float* dww, const float* dwb, int dw_act, int k, int st, int dil,
                  hipStream_t s);
// sparse_box.hip: the launches of the sparse box path's class tail, in a translation unit (and device code object) of
// their own.  Arguments with sk_deferred(), k 3 / stride 1 / 64 outputs (ds_check).
//   ds_defer_tile   the chunked kernel's tile (th x 8, cseg, dbuf) as launch_ds_tile picks it; false: no such instance
//   lean_defer_tile the one-round-trip 64 -> 64 tile
//   ds_zero_counts_masks  the counter-zeroing kernel that also zeroes the tile masks
bool ds_defer_tile(const ConvArgs<_Float16>& a, const float* dww, const float* dwb, int dw_act, int th, int cseg,
                   bool dbuf, hipStream_t s);
void lean_defer_tile(const ConvArgs<_Float16>& a, const float* dww, const float* dwb, int dw_act, hipStream_t s);
void ds_zero_counts_masks(int* counts, int n, unsigned char* masks, int nbytes, hipStream_t s);

template <typename T>
__device__ __forceinline__ f32x4 mfma_chunk(const typename Vec<T>::type& a, const typename Vec<T>::type& b, f32x4 c);

template <>
__device__ __forceinline__ f32x4 mfma_chunk<_Float16>(const h8& a, const h8& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma_chunk<float>(const f32x4& a, const f32x4& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
  return c;
}

// one MFMA k-step on policy operands (fp8: v_mfma_f32_16x16x32_fp8_fp8, 8 e4m3 per lane)
template <typename T, bool Q8>
__device__ __forceinline__ f32x4 mfma_op(const typename Op<T, Q8>::lds& a, const typename Op<T, Q8>::lds& b, f32x4 c) {
  if constexpr (Q8) return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((long)a, (long)b, c, 0, 0, 0);
  else return mfma_chunk<T>(a, b, c);
}

// The workgroup's N output channels' bias from c0 on, for the epilogue to read from LDS (conv_epilogue's sb):
// read from global memory after the k-loop, the bias cost every launch one more dependent round trip at its very
// end.  fetch() issues the loads at the start of the first round trip, commit() stores them into LDS just before
// that round trip's barrier (a store right after its load would wait on every load issued before it).  256-thread
// workgroups; clamped like the epilogue's own loads.
template <int N>
struct BiasStage {
  static constexpr int IT = (N + 255) / 256;
  float v[IT];
  __device__ __forceinline__ void fetch(const float* bias, int c0, int cout) {
#pragma unroll
    for (int it = 0; it < IT; ++it) v[it] = bias ? bias[min(c0 + (int)threadIdx.x + it * 256, cout - 1)] : 0.f;
  }
  __device__ __forceinline__ void commit(float* s) const {
#pragma unroll
    for (int it = 0; it < IT; ++it)
      if ((int)threadIdx.x + it * 256 < N) s[threadIdx.x + it * 256] = v[it];
  }
};

// Epilogue of one wave's TN x TM accumulator tiles: lane owns output channels co[i]..co[i]+3 of
// pixel pp[j].  Every load is unconditional from a clamped address (bias once; the residual of a
// pixel for all TN tiles at once) so the loads overlap; only the stores are predicated.
// sb: the bias staged in LDS for channels sb0.. (16-byte aligned), or nullptr to load it here.
// A: the activation (a code, or ACT_RT: p.act at run time).  R: the residual mode (a code, or -1: p.res at run
// time).  LEAN: Cout % 4 == 0 and no second output, so a lane's four channels are in range together and nothing
// but the y store follows.  conv_epilogue() below picks the form once per wave.
template <typename T, int TN, int TM, bool Q8, int A, int R, bool LEAN>
__device__ __forceinline__ void conv_epilogue_as(const ConvArgs<T>& p, const f32x4 (&acc)[TN][TM],
                                                 const int64_t (&pp)[TM], const bool (&pv)[TM], const int (&co)[TN],
                                                 const float* sb, int sb0) {
  const bool c4 = LEAN || (p.Cout & 3) == 0;  // uniform: co..co+3 in range whenever co < Cout
  const int res = R < 0 ? p.res : R;
  float bv[TN][4];
#pragma unroll
  for (int i = 0; i < TN; ++i) {
    if (sb) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(sb + co[i] - sb0);
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[i][q] = b4[q];
    } else if (p.bias) {
      if (c4) {
        load_f<4>(p.bias + min(co[i], p.Cout - 4), bv[i]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) bv[i][q] = p.bias[min(co[i] + q, p.Cout - 1)];
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[i][q] = 0.f;
    }
  }
  float dqv[TN][4];  // fp8 dequant factors (constant 1 folds away in the f16/f32 paths)
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) dqv[i][q] = Q8 ? p.dq[min(co[i] + q, p.Cout - 1)] : 1.f;
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    const int64_t pc = pv[j] ? pp[j] : 0;
    float rv[TN][4];
    if (res != YDBL_RES_NONE) {
      const T* rp = p.r + pc * p.rcs;
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        if (c4) {
          load_f<4>(rp + min(co[i], p.Cout - 4), rv[i]);
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) rv[i][q] = float(rp[min(co[i] + q, p.Cout - 1)]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      // the compiled forms are straight-line code: without a fence per fragment the scheduler interleaves the
      // activations of all TN x TM fragments, which cost the igemm and tile kernels 6-15 VGPRs and a wave per SIMD
      if constexpr (A != ACT_RT) __builtin_amdgcn_sched_barrier(0);
      float v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = act_as<T, A>(acc[i][j][q] * dqv[i][q] + bv[i][q], p.act);
      if (res == YDBL_RES_ADD) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = A == ACT_RT ? rv[i][q] + v[q] : add_rn(rv[i][q], v[q]);
      } else if (res == YDBL_RES_MUL) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = rv[i][q] * v[q];
      }
      if (!pv[j] || co[i] >= p.Cout) continue;
      T* yp = p.y + pc * p.ycs + co[i];
      if (LEAN || co[i] + 4 <= p.Cout) {
        store_f<4>(yp, v);
      } else {
        for (int q = 0; q < 4 && co[i] + q < p.Cout; ++q) store_f<1>(yp + q, v + q);
      }
      if (!LEAN && p.y2) {  // uniform
        const T* r2p = p.r2 + pc * p.r2cs + co[i];
        T* y2p = p.y2 + pc * p.y2cs + co[i];
        if (co[i] + 4 <= p.Cout) {
          float r2v[4];
          load_f<4>(r2p, r2v);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            r2v[q] = pad_mix(p.a2, round_to<T>(v[q]), p.b2, r2v[q]);  // y as stored (rounded to T)
          }
          store_f<4>(y2p, r2v);
        } else {
          for (int q = 0; q < 4 && co[i] + q < p.Cout; ++q) {
            const float o = pad_mix(p.a2, round_to<T>(v[q]), p.b2, float(r2p[q]));
            store_f<1>(y2p + q, &o);
          }
        }
      }
    }
  }
}

// The form of the epilogue, decided once per wave from the wave-uniform arguments: the common launches (SiLU or
// no activation, residual none or add, Cout % 4 == 0, one output) run straight-line code compiled for them; all
// others, and every launch under YDBL_EPI_GENERIC=1, run the form that tests the arguments where they are used.
// KA: ACT_ANY decides here, in the kernel.  The block-GEMM and spatial-tile kernels, whose accumulators live in
// AGPRs, are instead compiled per form and chosen on the host (epi_host_form): with both forms in one kernel the
// register allocator copies the whole accumulator to VGPRs ahead of the dispatch (128x64 igemm 59 -> 70 VGPRs,
// 5 -> 4 waves per SIMD).  KA = ACT_RT: the runtime form only; a code: that activation, preconditions host-checked.
constexpr int ACT_ANY = -2;
template <typename T>
inline int epi_host_form(const ConvArgs<T>& a) {
  if (sizeof(T) != 2 || a.epi_generic || (a.Cout & 3) || a.y2 || a.res == YDBL_RES_MUL) return ACT_RT;
  return a.act == YDBL_ACT_SILU || a.act == YDBL_ACT_NONE ? a.act : ACT_RT;
}
template <typename T, int TN, int TM, bool Q8 = false, int KA = ACT_ANY>
__device__ __forceinline__ void conv_epilogue(const ConvArgs<T>& p, const f32x4 (&acc)[TN][TM],
                                              const int64_t (&pp)[TM], const bool (&pv)[TM], const int (&co)[TN],
                                              const float* sb = nullptr, int sb0 = 0) {
  if constexpr (KA == ACT_RT) {
    conv_epilogue_as<T, TN, TM, Q8, ACT_RT, -1, false>(p, acc, pp, pv, co, sb, sb0);
  } else if constexpr (KA != ACT_ANY) {
    if (p.res == YDBL_RES_ADD) conv_epilogue_as<T, TN, TM, Q8, KA, YDBL_RES_ADD, true>(p, acc, pp, pv, co, sb, sb0);
    else conv_epilogue_as<T, TN, TM, Q8, KA, YDBL_RES_NONE, true>(p, acc, pp, pv, co, sb, sb0);
  } else {
    const bool lean = !std::is_same<T, float>::value && !p.epi_generic && (p.Cout & 3) == 0 && !p.y2 && p.res != YDBL_RES_MUL;
    if (lean && p.act == YDBL_ACT_SILU) {
      if (p.res == YDBL_RES_ADD) conv_epilogue_as<T, TN, TM, Q8, YDBL_ACT_SILU, YDBL_RES_ADD, true>(p, acc, pp, pv, co, sb, sb0);
      else conv_epilogue_as<T, TN, TM, Q8, YDBL_ACT_SILU, YDBL_RES_NONE, true>(p, acc, pp, pv, co, sb, sb0);
    } else if (lean && p.act == YDBL_ACT_NONE) {
      if (p.res == YDBL_RES_ADD) conv_epilogue_as<T, TN, TM, Q8, YDBL_ACT_NONE, YDBL_RES_ADD, true>(p, acc, pp, pv, co, sb, sb0);
      else conv_epilogue_as<T, TN, TM, Q8, YDBL_ACT_NONE, YDBL_RES_NONE, true>(p, acc, pp, pv, co, sb, sb0);
    } else {
      conv_epilogue_as<T, TN, TM, Q8, ACT_RT, -1, false>(p, acc, pp, pv, co, sb, sb0);
    }
  }
}

// Stores one pixel's class logits (part: the four lane groups' sums, equal on the pixel's four lanes g = 0..3)
// and, with a candidate sink, offers the pixel as an anchor: the four lanes are the decode's quad (lane g = side g
// and class g), the logits are taken as stored (the decode reads the fp16 values), and the level's box launch has
// run before this one, so a quad that holds a candidate reads its 64 box logits from the level buffer.
// SINK_DEFER: the level's box launch runs after this one; the quad flags its tile instead of decoding (decode_math.hpp).
template <typename T, int SINK>
__device__ __forceinline__ void tail_store(const ConvArgs<T>& p, const float (&part)[4], int64_t pix, bool ok, int g) {
  T lv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) lv[k] = T(part[k] + (k < p.nt3 ? p.t3b[k] : 0.f));
  if (g == 0 && ok) {
    T* o = p.y3 + pix * p.y3cs;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < p.nt3) o[k] = lv[k];
  }
  if constexpr (SINK && sizeof(T) == 2) {
    if (p.sk.ccount) {  // uniform
      const int hw = p.Ho * p.Wo;
      const int b = (int)pix / hw, loc = (int)pix - b * hw;
      const int gy = loc / p.Wo, gx = loc - gy * p.Wo;
      auto logit = [&](int j) { return float(j == 0 ? lv[0] : j == 1 ? lv[1] : j == 2 ? lv[2] : lv[3]); };
      if constexpr (SINK == SINK_DEFER) {
        unsigned char* tile = p.sk_mask(b, gy, gx);  // written only where ok
        quad_candidates<T, 16, true>(p.sk, b, g, ok, p.nt3, logit, static_cast<const T*>(nullptr), gx, gy,
                                     p.skstride, p.ska0 + loc, tile);
      } else {
        quad_candidates<T, 16>(p.sk, b, g, ok, p.nt3, logit, p.skbox + pix * p.skboxcs, gx, gy, p.skstride,
                               p.ska0 + loc);
      }
    }
  }
}

// Trailing 1x1 conv with <= 4 outputs over all Cout channels of a pixel, for kernels whose wave holds
// every channel of its pixels (TN * 16 == Cout): the Detect head's class conv cv3[i][2] (head.py:93-101)
// after its DWConv -> Conv1x1 pair.  Lane (r16, g) holds channels co[i]..co[i]+3 of pixel pp[j]; the
// rounded activations (T, as the unfused path stores them) are dotted with the weights per lane and the
// four lane groups are summed by xor-shuffles (fixed order); lane group 0 stores.
// SINK: the instance also serves a candidate sink (tail_store); the others are the plain tail, instruction for
// instruction.
template <typename T, int TN, int TM, int SINK = SINK_NONE>
__device__ __forceinline__ void conv_tail_1x1(const ConvArgs<T>& p, const f32x4 (&acc)[TN][TM], const int64_t (&pp)[TM],
                                              const bool (&pv)[TM], const int (&co)[TN], int g) {
  float bv[TN][4], wv[TN][4][4];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      bv[i][q] = p.bias ? p.bias[co[i] + q] : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) wv[i][q][k] = k < p.nt3 ? p.t3w[k * p.Cout + co[i] + q] : 0.f;
    }
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float u = round_to<T>(apply_act<T>(acc[i][j][q] + bv[i][q], p.act));  // y as stored
#pragma unroll
        for (int k = 0; k < 4; ++k) part[k] = fmaf(u, wv[i][q][k], part[k]);
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      part[k] += __shfl_xor(part[k], 16);
      part[k] += __shfl_xor(part[k], 32);
    }
    tail_store<T, SINK>(p, part, pp[j], pv[j], g);
  }
}

// The same tail from the values the epilogue stored (ys = y rounded to T, per lane [TN][TM][4]): no activation
// recomputed.  Lanes of one pixel share pv, so the xor-shuffles only mix lanes of the same pixel.
// s_t: the weights [4][Cout] staged in LDS (rows past nt3 zero), or nullptr to read them from global memory (a
// late round trip of 16 x nt3 scalar loads per lane at the very end of the launch: kbench pair 64+tail @80^2 bs16 24.8 vs 20.5 us, profiles/r05/r05_bias_lds_ab.txt).
template <typename T, int TN, int TM, int SINK = SINK_NONE>
__device__ __forceinline__ void conv_tail_1x1_vals(const ConvArgs<T>& p, const float (&ys)[TN][TM][4],
                                                   const int64_t (&pp)[TM], const bool (&pv)[TM], const int (&co)[TN],
                                                   int g, const float* s_t = nullptr) {
  float wv[TN][4][4];
  if (s_t) {
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(s_t + k * p.Cout + co[i]);
#pragma unroll
        for (int q = 0; q < 4; ++q) wv[i][q][k] = w4[q];
      }
  } else {
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[i][q][k] = k < p.nt3 ? p.t3w[k * p.Cout + co[i] + q] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    float part[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int k = 0; k < 4; ++k) part[k] = fmaf(ys[i][j][q], wv[i][q][k], part[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      part[k] += __shfl_xor(part[k], 16);
      part[k] += __shfl_xor(part[k], 32);
    }
    tail_store<T, SINK>(p, part, pp[j], pv[j], g);
  }
}

}  // namespace ydbl
