// Fused Bottleneck (fp16): y = x + SiLU(conv3x3(SiLU(conv3x3(x) + b1)) + b2)   (add = shortcut && c1 == c2)
// U/nn/modules/block.py:344-357 with Conv = conv + folded BN + SiLU (U/nn/modules/conv.py:39-63).
//
// The DBL backbones run chains of Bottleneck(C, C, e=0.5) at high resolution (DBL-n: C=16 @320^2,
// 32 @160^2, 4x 64 @80^2).  As two launches the C/2-channel intermediate is written to HBM and read
// back, and each 3x3 conv stages its own input; the pair is ~0.45 ms of DBL-n's 2.8 ms step.  Here a
// workgroup owns a TH x 16 output tile and all C output channels:
//   1. the (TH+4) x 20 input window, all C channels, is staged once in LDS (16-byte records, one plane
//      per 8-channel chunk; the lane -> (pixel, chunk) order gives 1 KiB contiguous global reads per
//      wave and conflict-free ds_write_b128 groups);
//   2. cv1 over the (TH+2) x 18 intermediate window on MFMA 16x16x32 f16, walked as a virtual grid with
//      the input's 20-record pitch (the two dead columns per row cost 11 %, and a lane's B address is
//      its pixel index plus a per-k-step constant), + bias + SiLU, zero outside the image (cv2's
//      padding), rounded to fp16 exactly as the unfused path stores it -> LDS;
//   3. cv2 over the TH x 16 tile from that LDS window, + bias + SiLU, + x (read back from the staged
//      input window), -> NHWC fp16.
// Weights never touch LDS: each wave keeps the MFMA A fragments of its output-channel tile in VGPRs
// (one 1 KiB coalesced load per k-step, every weight read once per workgroup).
// K order per 32-wide k-step (lane group g = lane / 16 supplies k = 8g..8g+7): chosen per channel
// count so that the two lane groups a ds_read_b128 services together ({g0, g1}, {g2, g3}) read from
// addresses 256 B apart (same bank quad offset): for >= 32 channels a k-step is one tap x 4 chunks, for
// 16 channels two taps x 2 chunks, for 8 channels four taps paired by equal dx (planes/pitches are
// multiples of 16 records).  Pack (host) and kernel share kslot().
// HBM traffic: x once (+ the 4-row halo, mostly L2 hits), y once; the intermediate never leaves LDS.
#include "bneck_kernel.hpp"

using namespace ydbl;

// (c, c_mid) pairs built: the backbone Bottleneck(c, c, e=0.5) chains and the Detect head's box
// branch cv2[i][0:2] = Conv(64, 64, 3) -> Conv(64, 64, 3) (head.py:86-90, no shortcut).
static int64_t pair_bytes(int c, int cm) {
  if (c == 16 && cm == 8) return BneckCfg<16, 8, 16>::BYTES;
  if (c == 32 && cm == 16) return BneckCfg<32, 16, 16>::BYTES;
  if (c == 64 && cm == 32) return BneckCfg<64, 32, 16>::BYTES;
  if (c == 64 && cm == 64) return BneckCfg<64, 64, 16>::BYTES;
  return -1;
}

#ifdef YDBL_BNECK_STAMPS
extern "C" int ydbl_bneck_debug_stamps(unsigned long long* out, int32_t n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bn_stamps), (size_t)n * 8) == hipSuccess ? 0 : -1;
}
extern "C" int ydbl_bneck_debug_reset() {
  static unsigned long long zeros[8 * 16384];
  return hipMemcpyToSymbol(HIP_SYMBOL(g_bn_stamps), zeros, sizeof(zeros)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int64_t ydbl_bottleneck_params_size(int32_t c) { return pair_bytes(c, c / 2); }
extern "C" int64_t ydbl_conv3x3_pair_params_size(int32_t c, int32_t c_mid) { return pair_bytes(c, c_mid); }

extern "C" int ydbl_conv3x3_pair_pack(const float* w1, const float* b1, const float* w2, const float* b2, int32_t c,
                                      int32_t c_mid, void* out) {
  if (!w1 || !b1 || !w2 || !b2 || !out) return fail(YDBL_EINVAL, "bottleneck_pack: null pointer");
  auto* o = reinterpret_cast<unsigned char*>(out);
  if (c == 16 && c_mid == 8) { bneck_pack<16, 8>(w1, b1, w2, b2, o); return 0; }
  if (c == 32 && c_mid == 16) { bneck_pack<32, 16>(w1, b1, w2, b2, o); return 0; }
  if (c == 64 && c_mid == 32) { bneck_pack<64, 32>(w1, b1, w2, b2, o); return 0; }
  if (c == 64 && c_mid == 64) { bneck_pack<64, 64>(w1, b1, w2, b2, o); return 0; }
  return fail(YDBL_EINVAL, "bottleneck_pack: (c, c_mid) must be (16, 8), (32, 16), (64, 32) or (64, 64)");
}

// Detect box branch: the (c_in -> 64 -> 64) pair blob + the trailing 1x1's A fragments (k = 32m + 8g + j
// -> input channel, row = output channel) and its fp32 bias.  c_in 64 (P3 of DBL-n), 128 (P4).
template <int CIN>
static int64_t box_bytes() {
  return BneckCfg<64, 64, 16, CIN>::BYTES + (64 / 16) * (64 / 32) * 64 * 16 + 64 * 4;
}

extern "C" int64_t ydbl_detect_box_params_size(int32_t c_in, int32_t c) {
  if (c != 64) return -1;
  if (c_in == 64) return box_bytes<64>();
  if (c_in == 128) return box_bytes<128>();
  return -1;
}

template <int CIN>
static void box_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                     const float* b3, unsigned char* out) {
  bneck_pack<64, 64, CIN>(w1, b1, w2, b2, out);
  _Float16* f3 = reinterpret_cast<_Float16*>(out + BneckCfg<64, 64, 16, CIN>::BYTES);
  constexpr int NT3 = 4, KS3 = 2;
  for (int t = 0; t < NT3; ++t)
    for (int m = 0; m < KS3; ++m)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 8; ++j) {
          const int co = 16 * t + (lane & 15), ci = (m * 4 + (lane >> 4)) * 8 + j;
          f3[((t * KS3 + m) * 64 + lane) * 8 + j] = (_Float16)w3[co * 64 + ci];
        }
  float* fb3 = reinterpret_cast<float*>(f3 + NT3 * KS3 * 64 * 8);
  for (int i = 0; i < 64; ++i) fb3[i] = b3[i];
}

extern "C" int ydbl_detect_box_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                    const float* b3, int32_t c_in, int32_t c, void* out) {
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !out) return fail(YDBL_EINVAL, "detect_box_pack: null pointer");
  if (c != 64 || (c_in != 64 && c_in != 128)) return fail(YDBL_EINVAL, "detect_box_pack: (c_in, c) must be (64|128, 64)");
  auto* o = reinterpret_cast<unsigned char*>(out);
  if (c_in == 64) box_pack<64>(w1, b1, w2, b2, w3, b3, o);
  else box_pack<128>(w1, b1, w2, b2, w3, b3, o);
  return 0;
}

extern "C" int ydbl_bottleneck_pack(const float* w1, const float* b1, const float* w2, const float* b2, int32_t c,
                                    void* out) {
  return ydbl_conv3x3_pair_pack(w1, b1, w2, b2, c, c / 2, out);
}

template <int C, int CMID, int TH, bool PW = false, int CIN = C>
static int bneck_go(const ydbl_bottleneck_desc* d, hipStream_t s) {
  using Cfg = BneckCfg<C, CMID, TH, CIN>;
  const int tiles_x = (int)cdiv(d->y.w, Cfg::TW), tiles_y = (int)cdiv(d->y.h, TH);
  const int64_t nt = (int64_t)tiles_x * tiles_y * d->y.n;
  if (nt > 0x7fffffff) return fail(YDBL_EINVAL, "bottleneck: grid too large");
  auto x = dview<const _Float16>(d->x);
  auto y = dview<_Float16>(d->y);
  auto* p = reinterpret_cast<const unsigned char*>(d->params);
  if constexpr (PW)
    bneck_kernel<C, CMID, TH, false, true, CIN><<<(unsigned)nt, 256, 0, s>>>(x, y, p, tiles_x, tiles_y, (int)nt);
  else if (d->add)
    bneck_kernel<C, CMID, TH, true><<<(unsigned)nt, 256, 0, s>>>(x, y, p, tiles_x, tiles_y, (int)nt);
  else
    bneck_kernel<C, CMID, TH, false><<<(unsigned)nt, 256, 0, s>>>(x, y, p, tiles_x, tiles_y, (int)nt);
  return check_launch("ydbl_bottleneck_nhwc");
}

// sparse_box.hip: the sparse Detect box launch (descriptor already checked; x.c 64 or 128)
namespace ydbl {
int box_sparse_launch(const ydbl_bottleneck_desc* d, hipStream_t s);
}

// workgroups of a bneck_kernel instantiation resident per CU x the CUs (queried once per instantiation)
template <int C, int CMID, int TH>
static int64_t bneck_slots() {
  static int64_t slots = [] {
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, bneck_kernel<C, CMID, TH, true>, 256, 0) != hipSuccess)
      return (int64_t)0;
    return (int64_t)cus * per;
  }();
  return slots;
}

template <int C, int CMID>
static int bneck_dispatch(const ydbl_bottleneck_desc* d, hipStream_t s) {
  // 16-row tiles halve the halo recompute; 8-row tiles when 16-row ones leave the chip under-filled
  // (and always for c_mid = 64: its 16-row tile would need 102 KB of LDS, one workgroup per CU)
  const int64_t t16 = cdiv(d->y.h, 16) * cdiv(d->y.w, 16) * (int64_t)d->y.n;
  int th = d->tile_h ? d->tile_h : (t16 >= 1024 && CMID < 64 ? 16 : 8);
  if constexpr (C == 64 && CMID == 32) {
    // 9-row tiles (51 KB of LDS: still 3 workgroups per CU) when they take fewer rounds of the resident
    // workgroups: DBL-n's 80^2 Bottlenecks at bs16 are 800 8-row tiles on 768 slots -- a second round of 32 --
    // and 720 9-row ones in one (a round priced by its cv1 rows, TH + 2)
    if (!d->tile_h && th == 8) {
      const int64_t s8 = bneck_slots<C, CMID, 8>(), s9 = bneck_slots<C, CMID, 9>();
      const int64_t t8 = cdiv(d->y.h, 8) * cdiv(d->y.w, 16) * (int64_t)d->y.n;
      const int64_t t9 = cdiv(d->y.h, 9) * cdiv(d->y.w, 16) * (int64_t)d->y.n;
      if (s8 > 0 && s9 > 0 && cdiv(t9, s9) * 11 < cdiv(t8, s8) * 10) th = 9;
    }
    if (th == 9) return bneck_go<C, CMID, 9>(d, s);
  }
  return th == 16 ? bneck_go<C, CMID, 16>(d, s) : bneck_go<C, CMID, 8>(d, s);
}

extern "C" int ydbl_bottleneck_nhwc(const ydbl_bottleneck_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "bottleneck: null descriptor");
  if (!d->params) return fail(YDBL_EINVAL, "bottleneck: null parameters");
  if (check_view(&d->x, "bottleneck.x", true) || check_view(&d->y, "bottleneck.y", true)) return YDBL_EINVAL;
  if (d->x.dtype != YDBL_F16 || d->y.dtype != YDBL_F16) return fail(YDBL_EINVAL, "bottleneck: fp16 views only");
  const int c = d->c, cm = d->c_mid ? d->c_mid : d->c / 2;
  const int cin = d->x.c;
  if (d->y.c != c || (cin != c && !(d->pw && cin == 128)))
    return fail(YDBL_EINVAL, "bottleneck: y.c must equal c, and x.c too (except x.c 128 with pw)");
  if (d->x.n != d->y.n || d->x.h != d->y.h || d->x.w != d->y.w)
    return fail(YDBL_EINVAL, "bottleneck: x and y shapes differ");
  if (d->y.n < 1 || d->y.h < 1 || d->y.w < 1) return fail(YDBL_EINVAL, "bottleneck: empty input");
  if (d->tile_h != 0 && d->tile_h != 8 && d->tile_h != 16 && !(d->tile_h == 9 && c == 64 && cm == 32))
    return fail(YDBL_EINVAL, "bottleneck: tile_h must be 0, 8 or 16 (or 9 for (c, c_mid) = (64, 32))");
  if (d->x.ptr == d->y.ptr) return fail(YDBL_EINVAL, "bottleneck: in-place is not supported (halo reads)");
  hipStream_t s = as_stream(stream);
  if (d->tile_mask || d->cand_count) {  // the sparse Detect box launch
    if (!d->pw || c != 64 || cm != 64 || d->add || (d->tile_h != 0 && d->tile_h != 8))
      return fail(YDBL_EINVAL, "bottleneck: the tile mask / candidate sink need pw = 1 (c = c_mid = 64) and 8-row tiles");
    if (!d->tile_mask) return fail(YDBL_EINVAL, "bottleneck: the candidate sink needs the tile mask");
    if (d->cand_count && (!d->cand_box || !d->cand_idx || d->cand_cap < 1 || d->cand_cap >= (1 << 24) ||
                          d->anchor0 < 0 || d->nc < 1 || d->nc > 4))
      return fail(YDBL_EINVAL, "bottleneck: the candidate sink needs cand_box, cand_idx, 1 <= cand_cap < 2^24, "
                               "anchor0 >= 0 and 1 <= nc <= 4");
    return box_sparse_launch(d, s);
  }
  if (c == 16 && cm == 8) return bneck_dispatch<16, 8>(d, s);
  if (c == 32 && cm == 16) return bneck_dispatch<32, 16>(d, s);
  if (c == 64 && cm == 32) return bneck_dispatch<64, 32>(d, s);
  if (c == 64 && cm == 64) {
    if (d->tile_h == 16) return fail(YDBL_EINVAL, "bottleneck: c_mid 64 takes 8-row tiles only");
    if (d->pw) {
      if (d->add) return fail(YDBL_EINVAL, "bottleneck: pw (trailing 1x1) excludes the residual add");
      return cin == 128 ? bneck_go<64, 64, 8, true, 128>(d, s) : bneck_go<64, 64, 8, true>(d, s);
    }
    return bneck_go<64, 64, 8>(d, s);
  }
  if (d->pw) return fail(YDBL_EINVAL, "bottleneck: pw needs (c, c_mid) = (64, 64)");
  return fail(YDBL_EINVAL, "bottleneck: (c, c_mid) must be (16, 8), (32, 16), (64, 32) or (64, 64)");
}
