// Instance masks from prototypes and coefficients, gfx950: process_mask / process_mask_native with crop_mask and
// scale_masks (U/utils/ops.py:644-737) in one launch per batch.
//
// Per kept detection: m = coef . proto.float() in fp32 over the proto grid; then
//   crop_after = 0 (process_mask):        m * box indicator on the proto grid, bilinear (align_corners=False) resampling
//                                         of the source window to (out_h, out_w), > 0;
//   crop_after = 1 (process_mask_native): the window resampled first, the box indicator on the output grid, > 0.
// out_h, out_w equal to the window makes the resampling an identity (scale 1, weights 1 and 0): upsample=False.
//
// Grid (output tiles of 32 rows x 64 columns, detection slot, image); a slot at or past count[image] writes nothing.
// A workgroup first finds the source rectangle its tile interpolates from (the source index is monotonic in the
// output index, so the tile's first and last pixel give it -- computed by the same function the pixels use).  If the
// box cannot touch the tile (crop_after = 0: no source pixel of the rectangle inside the scaled box; 1: no output pixel
// of the tile inside the box) it only stores zeros, in 16-byte chunks.  Otherwise it stages the rectangle's values
// (coef . proto, cropped when crop_after = 0) in LDS once, one source pixel per thread, and every output pixel
// interpolates from there; a
// rectangle larger than the LDS buffer (a strongly downsampling call) is evaluated per output pixel instead, the
// same arithmetic.  A thread owns 4 consecutive output columns: one 16-byte (fp32) or 4-byte (uint8) store where the
// address is aligned and the row holds all four, single stores otherwise.  No atomics, every output element of a live
// slot written exactly once: bit-identical from run to run.
//
// YDBL_MASK_BITS packs the same 0 / 1 values 64 columns to a uint64 word (bit j of word q = column 64 q + j, bits past
// out_w zero): a tile row is one word.  A thread shifts its four columns' nibble to its place, the 16 lanes of the row
// OR their words together with four __shfl_xor and the first of them stores; an untouched tile stores zero words.
//
// Bilinear follows torch's upsample_bilinear2d: scale = float(in) / out, src = max(scale * (d + 0.5) - 0.5, 0),
// i0 = int(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1,
// v = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11).
#include "common.hpp"

namespace ydbl {
namespace {

constexpr int MK_TH = 32, MK_TW = 64;  // output tile
constexpr int MK_SRC = 4096;           // staged source values (16 KiB)
constexpr int MK_NM = 64;              // most coefficients

struct MaskArgs {
  const void* proto; int mh, mw, nm, pcs;
  const void* mc[3]; int lh[3], lw[3], lcs[3], ldt[3]; int nl;
  const int* keep_idx; int nc;
  const float* det; int64_t det_stride; int det_row;
  const int* count;
  const float* coef;
  const int64_t* row_offset;
  void* out; int out_h, out_w;
  int top, left, wh, ww;  // source window: first row / column and extent
  float sx, sy; int crop_after;
  int max_det;
  int tiles_x;
};

// torch's area_pixel_compute_source_index (align_corners=False, not cubic); each operation rounded on its own
__device__ __forceinline__ float mk_src(float scale, int d) {
#pragma clang fp contract(off)
  const float t = scale * (float(d) + 0.5f);
  const float s = t - 0.5f;
  return s < 0.f ? 0.f : s;
}

template <typename T>
__device__ __forceinline__ float mk_dot(const T* p, const float* cf, int nm) {
  float acc = 0.f;
  for (int k = 0; k < nm; k += 8) {
    float v[8];
    load_f<8>(p + k, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = __builtin_fmaf(cf[k + i], v[i], acc);
  }
  return acc;
}

template <typename O>
__device__ __forceinline__ void mk_store4(O* row, int ox, int W, const bool* on) {
  O v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = on[i] ? O(1) : O(0);
  O* p = row + ox;
  if (ox + 3 < W && reinterpret_cast<uintptr_t>(p) % (4 * sizeof(O)) == 0) {
    if constexpr (sizeof(O) == 4) *reinterpret_cast<f32x4*>(p) = f32x4{float(v[0]), float(v[1]), float(v[2]), float(v[3])};
    else *reinterpret_cast<uchar4*>(p) = uchar4{(unsigned char)v[0], (unsigned char)v[1], (unsigned char)v[2], (unsigned char)v[3]};
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (ox + i < W) p[i] = v[i];
  }
}

template <typename T, typename O>
__global__ __launch_bounds__(256) void process_mask_kernel(MaskArgs a) {
  constexpr bool BITS = sizeof(O) == 8;  // O = uint64_t: bit planes, one word per tile row
  __shared__ float s_src[MK_SRC];
  __shared__ float s_cf[MK_NM];
  const int b = blockIdx.z, slot = blockIdx.y;
  if (slot >= min(a.count[b], a.max_det)) return;
  const int tid = threadIdx.x;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int oy0 = ty * MK_TH, ox0 = tx * MK_TW;
  const int oy1 = min(oy0 + MK_TH, a.out_h) - 1, ox1 = min(ox0 + MK_TW, a.out_w) - 1;  // last row / column, inclusive
  const int64_t ds = (int64_t)b * a.max_det + slot;
  const int64_t pitch = BITS ? a.tiles_x : a.out_w;  // elements of O per output row
  O* plane = reinterpret_cast<O*>(a.out) + (a.row_offset[b] + slot) * ((int64_t)a.out_h * pitch);

  const float* dr = a.det + (int64_t)b * a.det_stride + (int64_t)slot * a.det_row;
  float x1, y1, x2, y2;
  {
#pragma clang fp contract(off)
    x1 = dr[0] * a.sx; y1 = dr[1] * a.sy; x2 = dr[2] * a.sx; y2 = dr[3] * a.sy;
  }
  const float sch = float(a.wh) / float(a.out_h), scw = float(a.ww) / float(a.out_w);
  // the source rectangle of the tile, in window coordinates
  const int ry0 = min(int(mk_src(sch, oy0)), a.wh - 1), rx0 = min(int(mk_src(scw, ox0)), a.ww - 1);
  const int ry1 = min(min(int(mk_src(sch, oy1)), a.wh - 1) + 1, a.wh - 1);
  const int rx1 = min(min(int(mk_src(scw, ox1)), a.ww - 1) + 1, a.ww - 1);
  const int rw = rx1 - rx0 + 1, rh = ry1 - ry0 + 1;

  bool touched;
  if (a.crop_after)
    touched = float(ox1) >= x1 && float(ox0) < x2 && float(oy1) >= y1 && float(oy0) < y2;
  else
    touched = float(a.left + rx1) >= x1 && float(a.left + rx0) < x2 && float(a.top + ry1) >= y1 &&
              float(a.top + ry0) < y2;
  const int cg = (tid & 15) * 4, r0 = tid >> 4;  // this thread's 4 columns and first row within the tile
  if (!touched) {  // a NaN box lands here too: its indicator is false everywhere
    if constexpr (BITS) {
      if (tid < MK_TH && oy0 + tid <= oy1) plane[(int64_t)(oy0 + tid) * pitch + tx] = O(0);
      return;
    }
    // zeros in 16-byte chunks (4 fp32 / 16 uint8 elements) where the chunk is aligned and inside the row
    constexpr int NV = 16 / int(sizeof(O)), CPR = MK_TW / NV;  // elements per chunk, chunks per tile row
    for (int c = tid; c < MK_TH * CPR; c += 256) {
      const int oy = oy0 + c / CPR, ox = ox0 + (c % CPR) * NV;
      if (oy > oy1 || ox > ox1) continue;
      O* p = plane + (int64_t)oy * a.out_w + ox;
      if (ox + NV - 1 < a.out_w && reinterpret_cast<uintptr_t>(p) % 16 == 0) {
        *reinterpret_cast<f32x4*>(p) = f32x4{0.f, 0.f, 0.f, 0.f};  // (all-zero bits: 0.0f and 0 alike)
      } else {
        for (int i = 0; i < NV && ox + i < a.out_w; ++i) p[i] = O(0);
      }
    }
    return;
  }

  // coefficients: given directly, or the row of the level map the kept anchor names
  if (tid < a.nm) {
    float c = 0.f;
    if (a.coef) {
      c = a.coef[ds * a.nm + tid];
    } else {
      int idx = a.keep_idx[ds];
      if (a.nc > 0 && idx >= 0) idx /= a.nc;
      for (int l = 0; l < a.nl && idx >= 0; ++l) {
        const int hw = a.lh[l] * a.lw[l];
        if (idx < hw) {
          const int64_t e = ((int64_t)b * hw + idx) * a.lcs[l] + tid;
          c = a.ldt[l] == YDBL_F16 ? float(reinterpret_cast<const _Float16*>(a.mc[l])[e])
                                   : reinterpret_cast<const float*>(a.mc[l])[e];
          break;
        }
        idx -= hw;  // an index past the last level (or negative) leaves the coefficients zero
      }
    }
    s_cf[tid] = c;
  }
  __syncthreads();

  const T* pimg = reinterpret_cast<const T*>(a.proto) + (int64_t)b * a.mh * a.mw * a.pcs;
  auto source = [&](int i, int j) -> float {  // window coordinates -> coef . proto [* indicator]
    const int ay = a.top + i, ax = a.left + j;
    const float v = mk_dot<T>(pimg + ((int64_t)ay * a.mw + ax) * a.pcs, s_cf, a.nm);
    if (a.crop_after) return v;
    const bool in = float(ax) >= x1 && float(ax) < x2 && float(ay) >= y1 && float(ay) < y2;
    return in ? v : 0.f;
  };
  const bool staged = rw * rh <= MK_SRC;  // uniform over the workgroup
  if (staged) {
    for (int p = tid; p < rw * rh; p += 256) {
      const int i = p / rw, j = p - i * rw;
      s_src[p] = source(ry0 + i, rx0 + j);
    }
    __syncthreads();
  }
  auto value = [&](int i, int j) -> float { return staged ? s_src[(i - ry0) * rw + (j - rx0)] : source(i, j); };

  // this thread's 4 columns: source columns and weights, the same for every row
  int j0[4], j1[4];
  float w0[4], w1[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int ox = min(ox0 + cg + c, ox1);
    const float sxr = mk_src(scw, ox);
    j0[c] = min(int(sxr), a.ww - 1);
    j1[c] = min(j0[c] + 1, a.ww - 1);
    w1[c] = sxr - float(j0[c]);
    w0[c] = 1.f - w1[c];
  }
  if (!BITS && ox0 + cg > ox1) return;  // (bit planes: the row's 16 lanes all take part in its word)
  for (int r = r0; r < MK_TH; r += 16) {
    const int oy = oy0 + r;
    if (oy > oy1) break;
    const float syr = mk_src(sch, oy);
    const int i0 = min(int(syr), a.wh - 1), i1 = min(i0 + 1, a.wh - 1);
    const float h1 = syr - float(i0), h0 = 1.f - h1;
    bool on[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v00 = value(i0, j0[c]), v01 = value(i0, j1[c]), v10 = value(i1, j0[c]), v11 = value(i1, j1[c]);
      const float v = h0 * (w0[c] * v00 + w1[c] * v01) + h1 * (w0[c] * v10 + w1[c] * v11);
      bool o = v > 0.f;
      if (a.crop_after) {
        const float fx = float(ox0 + cg + c), fy = float(oy);
        o = o && fx >= x1 && fx < x2 && fy >= y1 && fy < y2;
      }
      on[c] = o;
    }
    if constexpr (BITS) {
      unsigned nib = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) nib |= (on[c] && ox0 + cg + c <= ox1 ? 1u : 0u) << c;
      unsigned long long w = (unsigned long long)nib << cg;  // oy is uniform over the row's 16 lanes
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) w |= __shfl_xor(w, m);
      if (cg == 0) plane[(int64_t)oy * pitch + tx] = w;
    } else {
      mk_store4<O>(plane + (int64_t)oy * a.out_w, ox0 + cg, a.out_w, on);
    }
  }
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_process_mask(const ydbl_mask_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "process_mask: null descriptor");
  if (int rc = check_view(&d->proto, "process_mask proto", true)) return rc;
  const int nm = d->proto.c;
  if (nm % 8 || nm > MK_NM) return fail(YDBL_EINVAL, "process_mask: nm must be a multiple of 8, at most 64");
  if (d->max_det < 1 || d->max_det > 4096) return fail(YDBL_EINVAL, "process_mask: max_det must be in [1, 4096]");
  if (!d->det || !d->count || !d->row_offset || !d->out) return fail(YDBL_EINVAL, "process_mask: null buffer");
  if (d->det_row != 0 && d->det_row < 4) return fail(YDBL_EINVAL, "process_mask: det_row must be 0 or >= 4");
  const int det_row = d->det_row ? d->det_row : 6;
  if (d->det_stride < 0 || (d->det_stride && d->det_stride < (int64_t)d->max_det * det_row))
    return fail(YDBL_EINVAL, "process_mask: det_stride must be 0 or >= max_det * det_row");
  if (d->out_h < 1 || d->out_w < 1) return fail(YDBL_EINVAL, "process_mask: empty output");
  if (d->out_dtype != YDBL_MASK_F32 && d->out_dtype != YDBL_MASK_U8 && d->out_dtype != YDBL_MASK_BITS)
    return fail(YDBL_EINVAL, "process_mask: out_dtype must be YDBL_MASK_F32, YDBL_MASK_U8 or YDBL_MASK_BITS");
  if (d->out_dtype == YDBL_MASK_BITS && reinterpret_cast<uintptr_t>(d->out) % 8)
    return fail(YDBL_EINVAL, "process_mask: a YDBL_MASK_BITS output must be 8-byte aligned");
  if (d->top < 0 || d->left < 0 || d->bottom <= d->top || d->right <= d->left || d->bottom > d->proto.h ||
      d->right > d->proto.w)
    return fail(YDBL_EINVAL, "process_mask: the source window must be a non-empty part of the proto grid");
  if (d->slots < 0 || d->slots > d->max_det) return fail(YDBL_EINVAL, "process_mask: slots must be in [0, max_det]");
  if (d->proto.n > 65535) return fail(YDBL_EINVAL, "process_mask: more than 65535 images");
  MaskArgs a{};
  a.proto = d->proto.ptr; a.mh = d->proto.h; a.mw = d->proto.w; a.nm = nm; a.pcs = d->proto.cs;
  if (d->coef) {
    a.coef = d->coef;
  } else {
    if (!d->keep_idx) return fail(YDBL_EINVAL, "process_mask: neither coef nor keep_idx");
    if (d->nl < 1 || d->nl > 3) return fail(YDBL_EINVAL, "process_mask: nl must be in [1, 3]");
    if (d->nc < 0) return fail(YDBL_EINVAL, "process_mask: nc must be >= 0");
    for (int l = 0; l < d->nl; ++l) {
      if (int rc = check_view(&d->mc[l], "process_mask mc", false)) return rc;
      if (d->mc[l].c != nm || d->mc[l].n != d->proto.n)
        return fail(YDBL_EINVAL, "process_mask: mc levels must be [n, h, w, nm]");
      if ((int64_t)d->mc[l].h * d->mc[l].w >= (int64_t)1 << 30) return fail(YDBL_EINVAL, "process_mask: level too large");
      a.mc[l] = d->mc[l].ptr; a.lh[l] = d->mc[l].h; a.lw[l] = d->mc[l].w; a.lcs[l] = d->mc[l].cs;
      a.ldt[l] = d->mc[l].dtype;
    }
    a.nl = d->nl; a.keep_idx = d->keep_idx; a.nc = d->nc;
  }
  a.det = d->det; a.det_row = det_row;
  a.det_stride = d->det_stride ? d->det_stride : (int64_t)d->max_det * det_row;
  a.count = d->count; a.row_offset = d->row_offset;
  a.out = d->out; a.out_h = d->out_h; a.out_w = d->out_w;
  a.top = d->top; a.left = d->left; a.wh = d->bottom - d->top; a.ww = d->right - d->left;
  a.sx = d->sx; a.sy = d->sy; a.crop_after = d->crop_after != 0;
  a.max_det = d->max_det;
  a.tiles_x = (int)cdiv(d->out_w, MK_TW);
  const int64_t tiles = (int64_t)a.tiles_x * cdiv(d->out_h, MK_TH);
  if (tiles >= (int64_t)1 << 31) return fail(YDBL_EINVAL, "process_mask: output too large");
  const dim3 grid((unsigned)tiles, (unsigned)(d->slots ? d->slots : d->max_det), (unsigned)d->proto.n);
  hipStream_t s = as_stream(stream);
  const bool h = d->proto.dtype == YDBL_F16, u8 = d->out_dtype == YDBL_MASK_U8;
  if (d->out_dtype == YDBL_MASK_BITS) {
    if (h) process_mask_kernel<_Float16, uint64_t><<<grid, 256, 0, s>>>(a);
    else process_mask_kernel<float, uint64_t><<<grid, 256, 0, s>>>(a);
  } else if (h && u8) process_mask_kernel<_Float16, uint8_t><<<grid, 256, 0, s>>>(a);
  else if (h) process_mask_kernel<_Float16, float><<<grid, 256, 0, s>>>(a);
  else if (u8) process_mask_kernel<float, uint8_t><<<grid, 256, 0, s>>>(a);
  else process_mask_kernel<float, float><<<grid, 256, 0, s>>>(a);
  return check_launch("ydbl_process_mask");
}
