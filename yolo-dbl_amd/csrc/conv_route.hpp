// The routing table of ydbl_conv2d_nhwc: which kernel family, template instance, split and grid a dense conv
// takes.  conv_route() is pure (nothing launched, nothing global read: the environment switches come in as a
// ConvSwitches record), so ydbl_conv_route and ydbl_conv_workspace (include/ydbl.h) answer from the same
// function the launch uses; conv.hip's launch() and conv3x3.hip's launch_conv3x3() only switch over the record.
#pragma once
#include <algorithm>

#include "conv_common.hpp"

namespace ydbl {

// The six A/B switches of the dense conv, read once per C-ABI call (conv.hip conv_switches) with each switch's own
// "off" value: '0' for YDBL_SPLITK, YDBL_HALO_SMALL and YDBL_WSK_HALF, '1' for YDBL_HALO_NB, YDBL_VW and
// YDBL_EPI_GENERIC; anything else is the default.
struct ConvSwitches {
  bool splitk;       // YDBL_SPLITK != 0: the split-K forms (halo and wave-split-K)
  bool halo_nb2;     // YDBL_HALO_NB != 1: two images per halo workgroup
  bool halo_small;   // YDBL_HALO_SMALL != 0: the small-map halo tile
  bool vw;           // YDBL_VW == 1: the VGPR-weight 3x3 kernel
  bool wsk_half;     // YDBL_WSK_HALF != 0: half-height wave-split-K tiles
  bool epi_generic;  // YDBL_EPI_GENERIC == 1: runtime-dispatch epilogues (ConvArgs::epi_generic)
};

// Everything a launch needs beyond ConvArgs: ydbl_conv_route_info as include/ydbl.h documents it (v[]: the template
// instance per family; workspace_bytes: the split-K partials this route writes).
using ConvRoute = ydbl_conv_route_info;

// conv3x3.hip: the launch of a YDBL_CONV_HALO or YDBL_CONV_VW route (a split route's partial tiles only; conv.hip's
// launch() runs the split-K epilogue kernel after it)
template <typename T, bool Q8>
void launch_conv3x3(const ConvRoute& r, const ConvArgs<T>& a, hipStream_t s);

// bytes of the fp32 partial tiles ws[ksplit][P][round_up(Cout, 4)] of a split-K launch, and "is there room"
template <typename T>
inline int64_t splitk_bytes(const ConvArgs<T>& a, int ksplit) {
  return ksplit > 1 ? (int64_t)ksplit * a.P * ((a.Cout + 3) & ~3) * 4 : 0;
}
template <typename T>
inline bool splitk_fits(const ConvArgs<T>& a, int ksplit) {
  return ksplit > 1 && a.ws && a.ws_bytes >= splitk_bytes(a, ksplit);
}

template <typename T>
inline ConvRoute make_route(const ConvArgs<T>& a, int family, int v0, int v1, int v2, int v3, int ksplit, int epi,
                            int64_t gx, int64_t gy = 1, int64_t gz = 1) {
  return ConvRoute{family, {v0, v1, v2, v3}, 0, ksplit, epi, {(uint32_t)gx, (uint32_t)gy, (uint32_t)gz},
                   splitk_bytes(a, ksplit)};
}

// fp16 3x3 stride-1 pad-1 convs routed to the VGPR-weight kernel; false when the shape is not one of
// them.  TPW output-channel tiles per wave, NWG wave groups over the channels (4 / NWG waves split the
// rows): combinations that fit 256 VGPRs without scratch (scripts/kres.py).
// Only the shapes where it measured faster than the halo / block-GEMM / tile kernels (conv_bench.py,
// bs32, MI355X): 128->64 @40^2 32.3 -> 21.3 us, 64->64 @40^2 20.0 -> 16.5 us.  Every workgroup loads
// all of its channels' weights into VGPRs, so on 80^2 maps (1600 workgroups) and for Cout 32/128 the
// re-read loses (measured with the kernel open to Cin/Cout 32..128: 64->64 @80^2 41.7 -> 47.9,
// 64->32 @80^2 22.5 -> 39.5, 64->128 @40^2 26.0 -> 29.4, 64->64 @20^2 8.9 -> 10.0 us).
inline bool route_vw(const ConvArgs<_Float16>& a, int kh, const ConvSwitches& sw, ConvRoute& r) {
  if (kh != 3 || a.KW != 3 || a.PAD != 1 || a.DIL != 1 || a.S != 1) return false;
  // Round 6: off by default -- the N-blocked halo tile takes these shapes (DBL-n bs32 +0.4 %, DBL-s bs8 +0.7 %, bs64
  // +1.5 %, profiles/r06/r06_conv_route_sweep.txt: less CU time per image in the two-branch layout, though each launch
  // is longer).  YDBL_VW=1 (read per launch) routes them here.
  if (!sw.vw) return false;
  if (a.xcs % 8 || a.H != a.Ho || a.W != a.Wo || (int64_t)a.N * a.Ho * a.Wo >= (1LL << 31)) return false;
  constexpr int64_t vw_min = 25601;
  const bool c128 = a.Cin == 128 && a.Cout == 64;
  if (!c128 && !(a.Cin == 64 && a.Cout == 64 && a.P >= vw_min && a.P <= 65536)) return false;
  // 8-row tiles, one output-channel slice: v = {Cin (the instance: 128 -> TPW 1, NWG 4; 64 -> TPW 2, NWG 2), rows}
  r = make_route(a, YDBL_CONV_VW, a.Cin, 8, 0, 0, 1, ACT_ANY, a.N * cdiv(a.Ho, 8) * cdiv(a.Wo, 16));
  return true;
}

// 3x3 / pad 1 / dil 1, Cin in {8,16,32}, Cout <= 64 and a multiple of 4: the spatial-tile kernel.
template <typename T>
inline bool route_tile(const ConvArgs<T>& a, int kh, ConvRoute& r) {
  if (kh != 3 || a.KW != 3 || a.DIL != 1 || a.PAD != 1 || a.Cout > 64 || a.Cout % 4) return false;
  if (a.S != 1 && a.S != 2) return false;
  if ((int64_t)a.Ho * a.Wo < 4096) return false;  // small maps: the GEMM kernel has more parallelism
  if (a.xcs % Vec<T>::N) return false;
  if (a.Cin != 8 && a.Cin != 16 && a.Cin != 32) return false;
  // 8 x 32 output tiles at stride 1, 8 x 16 at stride 2; the epilogue form is part of the kernel (conv_common.hpp,
  // conv_epilogue)
  r = make_route(a, YDBL_CONV_TILE, a.Cin, (a.Cout + 15) / 16, a.S, 0, 1, epi_host_form(a),
                 a.N * cdiv(a.Ho, 8) * cdiv(a.Wo, a.S == 1 ? 32 : 16));
  return true;
}

// Split-K of the halo kernel for the deep-K stride-1 convs on small maps (fewer than 25600 output pixels: the 40^2
// maps of a bs4 sub-batch), where a workgroup per tile leaves the chip idle behind a long serial chunk chain
// (DBL-s 768->128 @40^2 bs4: 24 chunks; on the wave-split-K kernel it took 53.7 us, its 32-pixel tiles re-reading the
// whole weight slice 200 times): up to 4 workgroups per tile over the input-channel chunks, >= 3 chunks each,
// toward 512 workgroups; the partials summed in split order by the epilogue kernel.
constexpr int HALO_SPLIT_MIN_CHUNKS = 8;
template <typename T>
inline int halo_ksplit(const ConvArgs<T>& a, int64_t wgs, const ConvSwitches& sw) {
  if (sizeof(T) != 2 || !sw.splitk) return 1;  // fp16 only (wsk_ksplit)
  const int nch = a.Cin / (4 * Vec<T>::N);
  if (nch < HALO_SPLIT_MIN_CHUNKS) return 1;
  int k = (int)std::min<int64_t>(4, (512 + wgs - 1) / wgs);
  while (k > 1 && nch / k < 3) --k;
  return k;
}

// 3x3, pad 1, dil 1, stride 1/2, Cin a multiple of BK and >= 2 chunks.  Returns false when the
// shape is not this kernel's (the caller falls back to the implicit-GEMM kernels).
// Where the halo tile beats the implicit GEMM (scripts/conv_bench.py, fp16, MI355X): stride 1 on
// >= 51200 output pixels.  Measured: 256->32 @80^2 bs32 132 -> 62 us, 512->64 @80^2 bs64
// 714 -> 382 us, 768->128 @40^2 bs64 534 -> 348 us, 1024->128 @160^2 bs8 1371 -> 688 us.
template <typename T>
inline bool route_halo(const ConvArgs<T>& a, int kh, bool q8, const ConvSwitches& sw, ConvRoute& r) {
  constexpr int BK = 4 * Vec<T>::N;
  if (kh != 3 || a.KW != 3 || a.PAD != 1 || a.DIL != 1 || (a.S != 1 && a.S != 2)) return false;
  if (a.Cin % BK || a.Cin < 2 * BK || a.xcs % Vec<T>::N) return false;
  // Stride 2 on >= 204800 output pixels: 8-row tiles over a (2*8+1) x 33 halo (A/B against the block
  // GEMM: DBL-l 128->256 @320 bs8 442 -> 341 us).  Smaller maps stay on the block GEMM: 128->128 @40 bs32
  // 17.8 vs 24.7 us, and DBL-n's 64->64 @80 bs32 (18.8 vs 17.5 us alone) cost the whole step ~40 us.
  if (a.S == 2 && (int64_t)a.P < 204800) return false;
  const int64_t tiles = cdiv(a.Ho, 8) * cdiv(a.Wo, 16), ntiles = a.N * tiles;  // 8-row x 16-column tiles (HALO_TH)
  // 51200 output pixels (40^2 x 32) was the measured crossover at bs32; the bench's two bs16 sub-batch
  // graphs put the 40^2 head convs at 25600, where the halo tile still wins (DBL-n bs32 on two streams
  // 13.7 k -> 14.1 k img/s; 12800 loses again: 14.0 k)
  // small maps: only as the split-K form (halo_ksplit), with room for its partials
  if (a.S == 1 && (int64_t)a.P < 25600) {
    const int64_t wgs = ntiles * cdiv(a.Cout, 32);  // (the split's own tiling: 32-channel slices)
    const int k = halo_ksplit(a, wgs, sw);
    if ((int64_t)a.P < 4096) return false;
    if (splitk_fits(a, k)) return r = make_route(a, YDBL_CONV_HALO, 1, 1, 32, 0, k, ACT_ANY, wgs, k), true;
    // Too few chunks to split (Cin < 256) and wide Cout: the wave-split-K kernel's 32x128 tiles would re-read the
    // whole weight matrix once per 32 pixels (DBL-s bs4: 128->256 @40^2, 200 tile rows x 590 KB); the halo tile in
    // 32-channel slices reads it once per 128 pixels
    // (YDBL_HALO_SMALL=0, read per launch: the wave-split-K route, A/B switch)
    if (!(k < 2 && a.Cout >= 128 && sw.halo_small)) return false;
  }
  // No 4-row tiles: every workgroup re-reads all of its channels' weights, so at 480 8-row tiles (40^2 bs32,
  // Cout 64) the doubled grid lost (A/B: 384->64 88.9 vs 49.6 us, 192->64 45.9 vs 28.0 us); 384->64 @40^2 also
  // beats the wave-split-K kernel it used to take (78.8 us).
  // Fewer than 400 64-channel workgroups (the 40^2 head convs of a bs16 sub-batch graph: 240) leave
  // most CUs with one workgroup; 32-channel slices double the grid (conv_bench.py bs16: 384->64 @40^2
  // 40.5 -> 29.5 us, 192->64 22.8 -> 17.3 us; at bs32, 480 workgroups, they lose: 49.2 -> 52.1 us)
  // (512: the 64->128 @40^2 head convs of a bs16 graph, 480 workgroups, also gain: 14.3 -> 13.2 us, kbench;
  // 16-channel slices and 4-row tiles lose on every head shape: profiles/r05/r05_halo_tile_ab.txt)
  constexpr int64_t n2_below = 512;
  // 8-row stride-1 tiles of two images per workgroup (N-blocking), 32-channel slices: half the weight staging per
  // output; each launch takes longer, but with less CU time the two sub-batch branches overlap better -- DBL-n bs32
  // +0.8 %, DBL-s bs64 / DBL-l 1280 bs8 +0.4 %, DBL-s bs8 even (profiles/r06/r06_fusion_switch_sweep.txt,
  // r06_sweep2.txt; per launch in graph at bs16: 384->64 @40^2 28.3 -> 33.5 us, 192->64 17.6 -> 20.2).
  // YDBL_HALO_NB=1 (read per launch; A/B switch): one image per workgroup.
  // (four images per workgroup, or two in 64-channel slices: DBL-n bs32 -3.1 / -2.3 %, r06_sweep3_cumask.txt)
  const int nb = a.S == 1 && !q8 && sw.halo_nb2 && a.N >= 2 ? 2 : 1;
  const int slice = nb == 2 || a.Cout <= 32 || ntiles * cdiv(a.Cout, 64) < n2_below ? 32 : 64;
  r = make_route(a, YDBL_CONV_HALO, a.S, nb, slice, 0, 1, ACT_ANY, cdiv(a.N, nb) * tiles * cdiv(a.Cout, slice));
  return true;
}

// The wave-split-K tiling (BM, BN).
// Under 256 workgroups with the usual tiles (the 20^2 maps of a bs16 sub-batch): half-height
// tiles, 16 pixels for Cout <= 64 and 64-wide columns for Cout 128 -- twice the workgroups for the same k-loop
// (bs16 graphs: 128->128 3x3 s2 @20^2 17.4 -> 14.4 us, 64->64 3x3 @20^2 9.5 -> 8.6, 256->64 18.4 -> 17.7; DBL-n
// bs32 even to +0.5 % over two boxes, DBL-s bs64 even: profiles/r04/r04_wsk_small_tiles_ab.txt); then the
// k-loop split where the tiles are still few (wsk_ksplit)
template <typename T>
inline void wsk_tiles(const ConvArgs<T>& a, const ConvSwitches& sw, int& bm, int& bn) {
  auto blocks = [&](int m, int n) { return cdiv(a.P, m) * cdiv(a.Cout, n); };
  const int64_t want = 768;
  // YDBL_WSK_HALF: A/B switch (read per launch): 0 = no half-height tiles
  const bool half = a.Cout <= 128 && blocks(32, a.Cout <= 64 ? 64 : 128) < 256 && sw.wsk_half;
  if (half) { bm = a.Cout <= 64 ? 16 : 32; bn = 64; return; }
  if (a.Cout <= 32) { bm = blocks(128, 32) >= want ? 128 : 64; bn = 32; return; }
  if (a.Cout <= 64) { bm = blocks(64, 64) >= want ? 64 : 32; bn = 64; return; }
  bm = 32;
  bn = blocks(32, 128) >= want || a.Cout % 128 == 0 ? 128 : 64;
}

// Split of the wave-split-K k-loop for a BM x BN tiling: the serial k-block chain is what a deep-K conv on a small
// map waits on (DBL-s bs4 sub-batch: 768->128 3x3 @40^2, 400 tiles of 54 k-block steps, about 1 us each: 53.7 us in
// graph), so below 768 tiles (3 workgroups per CU) the loop is split over up to 4 workgroups, each keeping >= 8
// steps.  YDBL_SPLITK=0 (read per launch): no split (A/B switch).
constexpr int WSK_SPLIT_BELOW = 768;
template <typename T>
inline int wsk_ksplit(const ConvArgs<T>& a, int bm, int bn, const ConvSwitches& sw) {
  if (sizeof(T) != 2 || !sw.splitk) return 1;  // fp16 only: the fp32 parity mode keeps one summation order
  const int64_t tiles = cdiv(a.P, bm) * cdiv(a.Cout, bn);
  const int nsteps = (int)cdiv(a.K, 16 * Vec<T>::N);  // BKB
  if (tiles >= WSK_SPLIT_BELOW || nsteps < 16) return 1;
  int k = (int)std::min<int64_t>(4, (WSK_SPLIT_BELOW + tiles - 1) / tiles);
  while (k > 1 && nsteps / k < 8) --k;
  return k;
}

// Wave-split-K where the block-tiled GEMM runs out of parallelism or k-depth per barrier:
// K >= 1024, or K >= 512 on small maps (measured on DBL-n: 384->64 3x3 @40^2 112 -> 82 us,
// 256->64 3x3 @20^2 47 -> 27 us; 64->64 3x3 @80^2 stays on conv_igemm_kernel, 47 vs 74 us).
template <typename T>
inline bool route_wsk(const ConvArgs<T>& a, const ConvSwitches& sw, ConvRoute& r) {
  if (!(a.K >= 1024 || (a.K >= 512 && a.P <= 16384))) return false;
  int bm, bn;
  wsk_tiles(a, sw, bm, bn);
  int k = wsk_ksplit(a, bm, bn, sw);
  if (!splitk_fits(a, k)) k = 1;  // no room: unsplit
  r = make_route(a, YDBL_CONV_WSK, bm, bn, 0, 0, k, ACT_ANY, cdiv(a.P, bm), cdiv(a.Cout, bn), k);
  return true;
}

// The block implicit GEMM's tile (BM x BN, waves as WM x WN).
template <typename T>
inline ConvRoute route_igemm(const ConvArgs<T>& a, bool pointwise, bool q8) {
  // BN covers Cout <= 64 in one column of workgroups (the input tile is then read once; wider Cout: below);
  // BM is the largest pixel tile that still gives >= `want` workgroups: 512 (2 per CU) for small
  // maps whose Cout fits one 128-wide column (bigger pixel tiles re-read the weights less:
  // 512->128 1x1 @40^2 bs32 31.3 -> 23.0 us, 384->128 25.6 -> 19.4 us), 1024 otherwise
  // (128->192: 16.4 vs 21.4 us; DBL-s bs64 end to end 0.8 % faster at 1024).
  // Shallow K (<= 128) on large maps: 2048 (8 per CU; each tile is a short k-loop, so more workgroups
  // hide each other's load latency: 64->128 @80^2 bs32 35.3 -> 28.1 us, 64->64 17.5 -> 16.4,
  // 128->64 22.2 -> 21.2).
  // (bs16 sub-batch graphs, scripts/kbench.py: for K 128, 2048 only above 131072 pixels -- 128->64 1x1 @80^2
  // 12.6 -> 11.3 us at 1024; K 64 keeps 2048 there, 64->128 @80^2 14.4 vs 15.6 us -- and 64x64 tiles for the
  // deep-K (>= 512) 3x3 convs with >= 16384 output pixels: 64->64 s2 @80^2 14.6 -> 13.1 us; DBL-n bs32 on two
  // streams 16.20 -> 16.30 k img/s over three pairs with the halo kernel's n2_below 512, DBL-s bs64 even)
  const int64_t want = a.Cout <= 128 && a.P <= 65536 ? 512
                       : (a.K <= 128 && a.P > (a.K <= 64 ? 65536 : 131072) ? 2048 : 1024);
  auto blocks = [&](int bm, int bn) { return cdiv(a.P, bm) * cdiv(a.Cout, bn); };
  int bm, bn;
  if (a.Cout <= 32) {
    bn = a.Cout <= 16 ? 16 : 32;
    bm = blocks(256, bn) >= want ? 256 : blocks(128, bn) >= want ? 128 : 64;
  } else {
    // (Cout <= 64: one column.)
    // Cout > 64: 64-wide column blocks (each workgroup stages half the weight rows; the input tile is read
    // once per column block, from L2/MALL at these map sizes).  Measured against 128-wide blocks on the
    // bench workloads: DBL-n bs32 14.82 -> 14.91 k img/s (bs16 graphs: 64->128 @80^2 22.6 -> 19.8 us,
    // 128->192 @40^2 15.6 -> 12.1 us), DBL-s bs64 7.52 -> 7.57 k, DBL-l 1280 bs8 467 -> 466 (noise).
    bn = 64;
    const bool deep3x3 = a.Cout <= 64 && !pointwise && a.K >= 512 && a.P >= 16384;
    bm = blocks(128, 64) >= want ? 128 : blocks(64, 64) >= want || deep3x3 ? 64 : 32;
  }
  // the epilogue form is part of the kernel (conv_common.hpp, conv_epilogue): fp16 SiLU / no activation compiled,
  // for the 1x1 convs (the general form of the 128x64 and 64x64 tiles would lose a wave per SIMD to it)
  const int epi = sizeof(T) == 2 && !q8 && pointwise ? epi_host_form(a) : ACT_RT;
  return make_route(a, YDBL_CONV_IGEMM, bm, bn, bn == 64 ? 2 : 4, bn == 64 ? 2 : 1, 1, epi, cdiv(a.P, bm),
                    cdiv(a.Cout, bn));
}

// Kernel choice: VGPR-weight 3x3 (fp16, behind YDBL_VW), thin-input spatial tile (f16/f32 only), halo tile,
// wave-split-K, block GEMM.  pointwise: 1x1 / stride 1 / pad 0 (the kernels' POINTWISE instances); q8: fp8 operands.
template <typename T>
inline ConvRoute conv_route(const ConvArgs<T>& a, int kh, bool pointwise, bool q8, const ConvSwitches& sw) {
  ConvRoute r;
  bool found = false;
  if constexpr (sizeof(T) == 2) found = !q8 && route_vw(a, kh, sw, r);
  found = found || (!q8 && route_tile(a, kh, r)) || route_halo(a, kh, q8, sw, r) || route_wsk(a, sw, r);
  if (!found) r = route_igemm(a, pointwise, q8);
  r.pointwise = pointwise;
  return r;
}

}  // namespace ydbl
