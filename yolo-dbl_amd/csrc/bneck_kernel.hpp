// The fused Bottleneck kernel of bneck.hip (design notes there), in a header because two translation units compile it:
//   bneck.hip          bneck_kernel -- the backbone Bottlenecks, the 64 -> 64 -> 64 pair and the Detect box launch;
//   sparse_box.hip     with YDBL_BNECK_SPARSE defined: bneck_sparse_kernel, the same body plus the tile mask and the
//                      candidate sink of the sparse box path.
// The preprocessor, not a template parameter, adds the sink: bneck_kernel keeps its name, its arguments and its code
// object whatever the sparse path grows into, and the sparse instances live in a code object of their own.
#pragma once
#include <algorithm>

#include "common.hpp"
#ifdef YDBL_BNECK_SPARSE
#include "decode_math.hpp"
#endif

namespace ydbl {

struct KSlot {
  int tap, chunk;
  bool live;
};

// k-step m, lane group g -> (tap = dy*3 + dx, 8-channel chunk, live); dead slots carry zero weights
// and point at a live address (finite data, broadcast reads)
template <int CH>
__host__ __device__ constexpr KSlot kslot(int m, int g) {
  if constexpr (CH >= 4) {
    return KSlot{m / (CH / 4), (m % (CH / 4)) * 4 + g, true};
  } else if constexpr (CH == 2) {
    const int tap = 2 * m + (g >> 1);
    return KSlot{tap < 9 ? tap : 8, g & 1, tap < 9};
  } else {
    // {g0,g1} and {g2,g3} share dx: (0,0)(1,0)|(0,1)(1,1), (0,2)(1,2)|(2,0)(2,0)', (2,1)(2,1)'|(2,2)(2,2)'
    constexpr int taps[3][4] = {{0, 3, 1, 4}, {2, 5, 6, 6}, {7, 7, 8, 8}};
    constexpr bool live[3][4] = {{true, true, true, true}, {true, true, true, false}, {true, false, true, false}};
    return KSlot{taps[m][g], 0, live[m][g]};
  }
}
template <int CH>
constexpr int ksteps() {
  return CH >= 4 ? 9 * CH / 4 : (CH == 2 ? 5 : 3);
}
constexpr int rup16(int v) { return (v + 15) / 16 * 16; }

template <int C, int CMID, int TH, int CIN = C>
struct BneckCfg {
  static constexpr int CM = CMID, CH = CIN / 8, CHM = (CM + 7) / 8;  // CH: 8-channel chunks of the input
  static constexpr int NT1 = (CM + 15) / 16, NT2 = C / 16;
  // BD (8-channel intermediate of a 16-channel input): cv1's 16 MFMA rows are two pixel sets x 8 channels through a
  // block-diagonal A (rows 0-7 see set 0's K slots, rows 8-15 set 1's), so no D row is dead; k-step m = tap m,
  // lane group g = (set g / 2, chunk g % 2)
  static constexpr bool BD = CM == 8 && CH == 2;
  static constexpr int KS1 = BD ? 9 : ksteps<CH>(), KS2 = ksteps<CHM>();
  static constexpr int TW = 16;
  static constexpr int IP = TW + 4;                  // input window pitch (records) = its width
  static constexpr int IR = TH + 5;                  // + 1 slack row for the virtual grid's tail
  static constexpr int NPX = IR * IP;
  static constexpr int PIN = rup16(NPX);             // chunk plane, records (multiple of 16: 256 B)
  static constexpr int MR = TH + 2;
  static constexpr int MP = CHM == 1 ? 32 : IP;      // 8-channel intermediate: pitch a multiple of 16
  static constexpr int PMID = rup16(MR * MP);
  static constexpr int G1 = (MR * IP + 15) / 16;     // 16-pixel groups of the cv1 virtual grid
  static constexpr int IN_BYTES = CH * PIN * 16, MID_BYTES = CHM * PMID * 16;
  static constexpr int LDS = IN_BYTES + MID_BYTES;
  static constexpr int W1F = NT1 * KS1 * 64, W2F = NT2 * KS2 * 64;  // h8 fragments
  static constexpr int64_t BYTES = (int64_t)(W1F + W2F) * 16 + (NT1 * 16 + C) * 4;
  static_assert(CH >= 2, "input needs >= 16 channels");
  static_assert((G1 * 16 - 1) + 2 * IP + 2 < NPX, "virtual grid tail must stay inside the window");
};

// Host: fp32 PyTorch-layout weights (BN folded) -> fragment blob.  A[row][k]: row = output channel of
// the 16-channel tile, k = 32m + 8g + j -> (kslot(m, g), channel chunk*8 + j).
template <int C, int CMID, int CIN = C>
void bneck_pack(const float* w1, const float* b1, const float* w2, const float* b2, unsigned char* out) {
  using Cfg = BneckCfg<C, CMID, 16, CIN>;
  constexpr int CM = Cfg::CM;
  _Float16* f1 = reinterpret_cast<_Float16*>(out);
  _Float16* f2 = f1 + Cfg::W1F * 8;
  float* fb1 = reinterpret_cast<float*>(f2 + Cfg::W2F * 8);
  float* fb2 = fb1 + Cfg::NT1 * 16;
  if constexpr (Cfg::BD) {
    for (int m = 0; m < Cfg::KS1; ++m)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int g = lane >> 4, row = lane & 15;
          const int co = row % 8, ci = (g & 1) * 8 + j;
          f1[(m * 64 + lane) * 8 + j] = (_Float16)((row / 8) == (g >> 1) ? w1[(co * CIN + ci) * 9 + m] : 0.f);
        }
  } else
  for (int t = 0; t < Cfg::NT1; ++t)
    for (int m = 0; m < Cfg::KS1; ++m)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const KSlot s = kslot<Cfg::CH>(m, lane >> 4);
          const int co = 16 * t + (lane & 15), ci = s.chunk * 8 + j;
          const bool ok = s.live && co < CM;
          f1[((t * Cfg::KS1 + m) * 64 + lane) * 8 + j] = (_Float16)(ok ? w1[(co * CIN + ci) * 9 + s.tap] : 0.f);
        }
  for (int t = 0; t < Cfg::NT2; ++t)
    for (int m = 0; m < Cfg::KS2; ++m)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const KSlot s = kslot<Cfg::CHM>(m, lane >> 4);
          const int co = 16 * t + (lane & 15), ci = s.chunk * 8 + j;
          const bool ok = s.live && ci < CM;
          f2[((t * Cfg::KS2 + m) * 64 + lane) * 8 + j] = (_Float16)(ok ? w2[(co * CM + ci) * 9 + s.tap] : 0.f);
        }
  for (int i = 0; i < Cfg::NT1 * 16; ++i) fb1[i] = i < CM ? b1[i] : 0.f;
  for (int i = 0; i < C; ++i) fb2[i] = b2[i];
}

// per-k-step LDS byte offset of lane group g's slot relative to its pixel record (PL = chunk plane,
// P = pitch, both in records); g-independent except for the lane base chunk when CH >= 4
template <int CH, int PL, int P>
__device__ __forceinline__ int koff(int m, int g) {
  const KSlot s = kslot<CH>(m, CH >= 4 ? 0 : g);
  return (s.chunk * PL + (s.tap / 3) * P + s.tap % 3) * 16;
}
template <int CH, int PL>
__device__ __forceinline__ int kbase(int g) {
  return CH >= 4 ? g * PL * 16 : 0;
}

// Diagnostic build only (-DYDBL_BNECK_STAMPS, scripts/phase_stamps.py): per-workgroup s_memrealtime stamps (100 MHz)
// when wave 0 starts, has staged the window, has finished cv1, has stored cv2; plus the hardware ids.
#if defined(YDBL_BNECK_STAMPS) && defined(YDBL_BNECK_SPARSE)
#undef YDBL_BNECK_STAMPS  // the stamps belong to bneck.hip's kernels
#endif
#ifdef YDBL_BNECK_STAMPS
__device__ unsigned long long g_bn_stamps[8 * 16384];
#define BN_STAMP(k)                                                                                         \
  do {                                                                                                    \
    if (threadIdx.x == 0 && blockIdx.x < 16384) g_bn_stamps[blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define BN_STAMP(k) \
  do {              \
  } while (0)
#endif

#ifdef YDBL_BNECK_SPARSE
// The sparse Detect box launch (include/ydbl.h, ydbl_bottleneck_desc tile_mask / candidate sink): one mask byte per
// tile in the kernel's own tile order, and the candidate lists the level's class tail has filled but for the boxes.
struct BoxSink {
  const unsigned char* mask;
  float* cbox;
  const int* cidx;
  const int* ccount;  // nullptr: mask only
  int cap, a0, nc, multi;
  float stride;
};
// LDS the sink needs in the intermediate window's space (free once cv2 has read it): the tile's 64 logits per pixel as
// stored (f16, pitch 72: 16-byte aligned rows, 4-bank skew), the tile's candidate list and its length
constexpr int BOX_PITCH = 72, BOX_HITS = 512;  // <= 128 pixels x nc <= 4 entries

#define YDBL_BNECK_KERNEL bneck_sparse_kernel
#define YDBL_BNECK_SINK_ARG , BoxSink sk
#else
#define YDBL_BNECK_KERNEL bneck_kernel
#define YDBL_BNECK_SINK_ARG
#endif

// bneck_sparse_kernel (PW only): a workgroup returns at once where its tile's mask byte is 0, and after the tile is
// stored decodes the boxes of the image's candidates that lie in it.
template <int C, int CMID, int TH, bool ADD, bool PW = false, int CIN = C>
__global__ __launch_bounds__(256, 2) void YDBL_BNECK_KERNEL(DView<const _Float16> x, DView<_Float16> y,
                                                            const unsigned char* __restrict__ params, int tiles_x,
                                                            int tiles_y, int ntiles YDBL_BNECK_SINK_ARG) {
  using Cfg = BneckCfg<C, CMID, TH, CIN>;
#ifdef YDBL_BNECK_SPARSE
  static_assert(PW, "the tile mask belongs to the Detect box launch");
#endif
  constexpr int CH = Cfg::CH, CHM = Cfg::CHM, CM = Cfg::CM;
  static_assert(CIN == C || !ADD, "the residual needs c_in == c");
  constexpr bool LATE_A2 = CIN > C;  // deep input: cv2's A fragments are loaded after cv1 (VGPR budget)
  constexpr int IP = Cfg::IP, MP = Cfg::MP, PIN = Cfg::PIN, PMID = Cfg::PMID;
  constexpr int NT1 = Cfg::NT1, NT2 = Cfg::NT2, KS1 = Cfg::KS1, KS2 = Cfg::KS2;
  const h8* w1f = reinterpret_cast<const h8*>(params);
  const h8* w2f = w1f + Cfg::W1F;
  const float* b1 = reinterpret_cast<const float*>(w2f + Cfg::W2F);
  const float* b2 = b1 + NT1 * 16;
  __shared__ __align__(16) unsigned char smem[Cfg::LDS];
  unsigned char* s_in = smem;                    // [CH][PIN] records
  unsigned char* s_mid = smem + Cfg::IN_BYTES;   // [CHM][PMID] records

  const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int g = lane >> 4, r16 = lane & 15;
  BN_STAMP(0);
#ifdef YDBL_BNECK_STAMPS
  if (tid == 0 && blockIdx.x < 16384) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_bn_stamps[blockIdx.x * 8 + 4] = hw;
    g_bn_stamps[blockIdx.x * 8 + 5] = xcc;
  }
#endif
  const int t = (ntiles & 7) ? (int)blockIdx.x : xcd_remap(blockIdx.x, ntiles);
  const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y;
  const int img = t / (tiles_x * tiles_y);
  const int oy0 = ty * TH, ox0 = tx * Cfg::TW;
#ifdef YDBL_BNECK_SPARSE
  if (sk.mask[t] == 0) return;  // (uniform) no candidate in this tile: nothing reads its box logits
  __shared__ int s_nhit;        // length of the tile's candidate list (zeroed here, two barriers ahead of its use)
  if (tid == 0) s_nhit = 0;
  int ncand = 0, idx0 = -1;     // the image's candidate count and this thread's entry of the first 256
  if (sk.ccount) {  // both loads issued ahead of the window loads (neither waits for the other), read after the 1x1
    ncand = min(sk.ccount[img], sk.cap);
    idx0 = sk.cidx[(int64_t)img * sk.cap + min(tid, sk.cap - 1)];
  }
#endif

  // ---- 1. input window (image rows oy0-2.., cols ox0-2..).  Item i = u*256 + tid -> chunk
  // (i >> 3) % CH (the same for every u: CH divides 32), pixel px0 + u * 256/CH: each wave reads
  // 1 KiB of contiguous NHWC pixels per instruction, each 8-lane ds_write_b128 group 8 records
  static_assert(32 % CH == 0, "staging pattern assumes CH | 32");
  constexpr int PXU = 256 / CH;
  constexpr int IT = (Cfg::NPX + PXU - 1) / PXU;
  const int s_chunk = (tid >> 3) % CH, px0 = ((tid >> 3) / CH) * 8 + (tid & 7);
  h8 xr[IT];
#pragma unroll
  for (int u = 0; u < IT; ++u) {
    const int px = px0 + u * PXU;
    const int r = px / IP, c = px - r * IP;
    const int iy = oy0 - 2 + r, ix = ox0 - 2 + c;
    const bool ok = px < Cfg::NPX && iy >= 0 && iy < x.h && ix >= 0 && ix < x.w;
    const _Float16* src = ok ? x.at(img, iy, ix) + s_chunk * 8 : x.p;
    const h8 v = *reinterpret_cast<const h8*>(src);
    xr[u] = ok ? v : h8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  // this wave's weight tiles, VGPR-resident
  const int t1 = wave % NT1, t2 = wave % NT2;
  h8 a1[KS1], a2[KS2];
#pragma unroll
  for (int m = 0; m < KS1; ++m) a1[m] = w1f[(t1 * KS1 + m) * 64 + lane];
  if constexpr (!LATE_A2) {
#pragma unroll
    for (int m = 0; m < KS2; ++m) a2[m] = w2f[(t2 * KS2 + m) * 64 + lane];
  }
  unsigned char* s_dst = s_in + (s_chunk * PIN + px0) * 16;
#pragma unroll
  for (int u = 0; u < IT; ++u)
    if (px0 + u * PXU < Cfg::NPX) *reinterpret_cast<h8*>(s_dst + u * PXU * 16) = xr[u];
  float bias1[4], bias2[4];
  const int c1 = Cfg::BD ? 4 * (g & 1) : 16 * t1 + 4 * g;  // first intermediate channel of this lane's cv1 D rows
  const int c2 = 16 * t2 + 4 * g;  // first output channel of this lane's cv2 D rows
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bias1[q] = b1[c1 + q];
    bias2[q] = b2[c2 + q];
  }
  unsigned char* mid_w = s_mid + ((c1 >> 3) * PMID) * 16 + (c1 & 7) * 2;
  const unsigned char* in_b = s_in + kbase<CH, PIN>(g);
  const bool interior = oy0 >= 1 && ox0 >= 1 && oy0 + TH + 1 <= y.h && ox0 + Cfg::TW + 1 <= y.w;
  __syncthreads();
  BN_STAMP(1);

  // ---- 2. cv1 over the virtual grid: MR rows x IP columns, mid pixel v reads input record v + tap.
  // Two 16-pixel groups per iteration (independent accumulators: the LDS reads of one overlap the
  // MFMAs of the other, and the two SiLU epilogues interleave)
  auto epi1 = [&](const f32x4& acc, int vr, int vc, int rb) {
    if (vr >= Cfg::MR || c1 >= CM) return;
    bool inside = true;
    if (!interior) {
      const int my = oy0 - 1 + vr, mx = ox0 - 1 + vc;
      inside = my >= 0 && my < y.h && mx >= 0 && mx < y.w;
    }
    h4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float sv = silu_fast(acc[q] + bias1[q]);  // computed unconditionally: a select, not a branch per value
      o[q] = f16_rne(inside ? sv : 0.f);
    }
    *reinterpret_cast<h4*>(mid_w + (rb + vc) * 16) = o;
  };
  constexpr int WPT1 = 4 / NT1;
  // the two groups' virtual-grid (row, column) and intermediate row base, walked incrementally (no division
  // or 32-bit multiply in the loop): group 0 advances S0 pixels per iteration, group 1 sits H1 pixels after it
  constexpr int S0 = 2 * WPT1 * 16, H1 = WPT1 * 16;
  int r0, c0, rb0;
  {
    const int v = (wave / NT1) * 16 + r16;
    r0 = v / IP;
    c0 = v - r0 * IP;
    rb0 = r0 * MP;
  }
  for (int gi = wave / NT1; gi < Cfg::G1; gi += 2 * WPT1) {
    const int v0 = gi * 16 + r16;
    const bool two = gi + WPT1 < Cfg::G1;  // wave-uniform
    const int v1 = two ? v0 + 16 * WPT1 : v0;
    if constexpr (Cfg::BD) {
      // one accumulator for both groups: lane group g reads set g / 2's pixel, chunk g % 2, at tap m
      const int set = g >> 1;
      const unsigned char* pb = s_in + ((g & 1) * PIN + (set ? v1 : v0)) * 16;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < KS1; ++m) {
        const h8 bf = *reinterpret_cast<const h8*>(pb + ((m / 3) * IP + m % 3) * 16);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[m], bf, acc, 0, 0, 0);
      }
      // one epilogue for both sets (per-lane position select, not a branch per set); set 1 of a single-group
      // iteration duplicates group 0 and is skipped through an out-of-range row
      const bool w1 = c0 + H1 % IP >= IP;
      const int dr = set ? H1 / IP + (w1 ? 1 : 0) : 0;
      epi1(acc, set && !two ? Cfg::MR : r0 + dr, set ? c0 + H1 % IP - (w1 ? IP : 0) : c0, rb0 + dr * MP);
    } else {
      f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
      const unsigned char* p0 = in_b + v0 * 16;
      const unsigned char* p1 = in_b + v1 * 16;
#pragma unroll
      for (int m = 0; m < KS1; ++m) {
        const int o = koff<CH, PIN, IP>(m, g);
        const h8 bf0 = *reinterpret_cast<const h8*>(p0 + o);
        const h8 bf1 = *reinterpret_cast<const h8*>(p1 + o);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[m], bf0, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[m], bf1, acc1, 0, 0, 0);
      }
      epi1(acc0, r0, c0, rb0);
      if (two) {
        const bool w1 = c0 + H1 % IP >= IP;
        const int dr = H1 / IP + (w1 ? 1 : 0);
        epi1(acc1, r0 + dr, c0 + H1 % IP - (w1 ? IP : 0), rb0 + dr * MP);
      }
    }
    const bool w0 = c0 + S0 % IP >= IP;
    const int dr = S0 / IP + (w0 ? 1 : 0);
    c0 += S0 % IP - (w0 ? IP : 0);
    r0 += dr;
    rb0 += dr * MP;
  }

  const unsigned char* res_r = s_in + ((c2 >> 3) * PIN + 2 * IP + 2) * 16 + (c2 & 7) * 2;
  const unsigned char* mid_b = s_mid + kbase<CHM, PMID>(g);
  if constexpr (LATE_A2) {
#pragma unroll
    for (int m = 0; m < KS2; ++m) a2[m] = w2f[(t2 * KS2 + m) * 64 + lane];
  }
  __syncthreads();
  BN_STAMP(2);

  // ---- 3. cv2: output rows j, j + WPT2 of the tile, 16 columns = the 16 lanes
  const int64_t lane_px = (int64_t)r16 * y.cs;  // this lane's pixel offset from the row's first column
  auto epi2 = [&](const f32x4& acc, int j) {
    const int oy = oy0 + j, ox = ox0 + r16;
    if (oy >= y.h || ox >= y.w) return;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = silu_fast(acc[q] + bias2[q]);
    if constexpr (ADD) {
      const h4 rv = *reinterpret_cast<const h4*>(res_r + (j * IP + r16) * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = float(rv[q]) + v[q];
    }
    if constexpr (PW) {  // cv2 output, rounded to fp16 as the unfused path stores it, -> LDS for the 1x1
      h4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = f16_rne(v[q]);
      *reinterpret_cast<h4*>(s_in + ((c2 >> 3) * (TH * 16) + j * 16 + r16) * 16 + (c2 & 7) * 2) = o;
    } else {
      store_f<4>(y.at(img, oy, ox0) + lane_px + c2, v);  // row base wave-uniform (scalar address arithmetic)
    }
  };
  constexpr int WPT2 = 4 / NT2;
  for (int j = wave / NT2; j < TH; j += 2 * WPT2) {
    const bool two = j + WPT2 < TH;
    const int j1 = two ? j + WPT2 : j;
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    const unsigned char* p0 = mid_b + (j * MP + r16) * 16;
    const unsigned char* p1 = mid_b + (j1 * MP + r16) * 16;
#pragma unroll
    for (int m = 0; m < KS2; ++m) {
      const int o = koff<CHM, PMID, MP>(m, g);
      const h8 bf0 = *reinterpret_cast<const h8*>(p0 + o);
      const h8 bf1 = *reinterpret_cast<const h8*>(p1 + o);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[m], bf0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2[m], bf1, acc1, 0, 0, 0);
    }
    epi2(acc0, j);
    if (two) epi2(acc1, j1);
  }
  BN_STAMP(3);

  if constexpr (PW) {
    // ---- 4. trailing 1x1 conv C -> C + bias (Detect box branch cv2[i][2], head.py:86-90) over the
    // TH x 16 cv2 tile now in LDS (C/8 planes of TH*16 records, in the input window's space)
    static_assert(ADD == false && C % 32 == 0 && (C / 8) * TH * 16 * 16 <= Cfg::IN_BYTES, "pw stage layout");
    constexpr int NT3 = C / 16, KS3 = C / 32, WPT3 = 4 / NT3;
    const h8* w3f = reinterpret_cast<const h8*>(b2 + C);
    const float* b3 = reinterpret_cast<const float*>(w3f + NT3 * KS3 * 64);
    const int t3 = wave % NT3, c3 = 16 * t3 + 4 * g;
    h8 a3[KS3];
#pragma unroll
    for (int m = 0; m < KS3; ++m) a3[m] = w3f[(t3 * KS3 + m) * 64 + lane];
    float bias3[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bias3[q] = b3[c3 + q];
    __syncthreads();
#ifdef YDBL_BNECK_SPARSE
    // the intermediate window is free from here on (every wave is past cv2) and holds the sink's copy
    _Float16* s_box = reinterpret_cast<_Float16*>(s_mid);
    int* s_hit = reinterpret_cast<int*>(s_mid + TH * 16 * BOX_PITCH * 2);  // [BOX_HITS]
    static_assert(C == 64 && TH * 16 * BOX_PITCH * 2 + BOX_HITS * 4 <= Cfg::MID_BYTES, "sink layout");
#endif
    for (int j = wave / NT3; j < TH; j += WPT3) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int m = 0; m < KS3; ++m) {
        const h8 bf = *reinterpret_cast<const h8*>(s_in + ((m * 4 + g) * (TH * 16) + j * 16 + r16) * 16);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a3[m], bf, acc, 0, 0, 0);
      }
      const int oy = oy0 + j, ox = ox0 + r16;
      if (oy < y.h && ox < y.w) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = acc[q] + bias3[q];
#ifdef YDBL_BNECK_SPARSE  // the same rounded values to y and to the copy the boxes are decoded from
        const h4 o = to_h4_rne(v);
        *reinterpret_cast<h4*>(y.at(img, oy, ox) + c3) = o;
        *reinterpret_cast<h4*>(s_box + (j * 16 + r16) * BOX_PITCH + c3) = o;
#else
        store_f<4>(y.at(img, oy, ox) + c3, v);
#endif
      }
    }
#ifdef YDBL_BNECK_SPARSE
    {
      // ---- 5. the boxes of this tile's candidates.  Scan: a thread per list entry (the first 256 were loaded at the
      // top), entries of this level and this tile -> s_hit as (slot << 7 | tile pixel).  Decode: a quad per hit, lane s
      // = side s, as the class tail's quad does it (decode_math.hpp), so the boxes are the box-first path's bits.
      if (sk.ccount == nullptr) return;  // (uniform)
      const int hw = y.h * y.w;
      const int* ci = sk.cidx + (int64_t)img * sk.cap;
      for (int i = tid; i < ncand; i += 256) {
        const int idx = i == tid ? idx0 : ci[i];
        const int loc = (sk.multi ? idx / sk.nc : idx) - sk.a0;
        if (loc < 0 || loc >= hw) continue;
        const int gy = loc / y.w, gx = loc - gy * y.w;
        const int jy = gy - oy0, jx = gx - ox0;
        if (jy < 0 || jy >= TH || jx < 0 || jx >= 16) continue;
        const int h = atomicAdd(&s_nhit, 1);
        if (h < BOX_HITS) s_hit[h] = (i << 7) | (jy * 16 + jx);
      }
      __syncthreads();  // the copy and the hit list are complete
      const int nh = min(s_nhit, BOX_HITS);
      const int s = tid & 3;
      for (int h0 = 0; h0 < nh; h0 += 64) {  // (uniform trip count: the shuffles see whole quads)
        const int h = h0 + (tid >> 2);
        const bool live = h < nh;
        const int e = s_hit[live ? h : 0];
        const int px = e & 127;
        const float mine = dfl_side(s_box + px * BOX_PITCH + s * 16);
        const int q0 = lane - s;
        float dist[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) dist[k] = __shfl(mine, q0 + k);
        const f32x4 box = xywh2xyxy(dist2xywh(ox0 + (px & 15), oy0 + (px >> 4), dist, sk.stride));
        if (live && s == 0) *reinterpret_cast<f32x4*>(sk.cbox + ((int64_t)img * sk.cap + (e >> 7)) * 4) = box;
      }
    }
#endif
  }
}

}  // namespace ydbl
