// scale_img: the resize + pad of test-time augmentation (U/utils/torch_utils.py:423-432 as DetectionModel.
// _predict_augment calls it, U/nn/tasks.py:361-376), with the optional left-right flip of the source folded in.
//
// y[:, :, :sh, :sw] = F.interpolate(x or x.flip(3), size=(sh, sw), mode="bilinear", align_corners=False); every
// other texel of y [n][c][hp][wp] = pad_value.  torch's fp32 rule (ATen UpSample.h area_pixel_compute_source_index
// + the linear kernel): scale = float(in) / float(out), src = max(scale * (dst + 0.5) - 0.5, 0) with the multiply
// and subtract as ONE fma (what ATen's vectorised CPU kernel computes; two roundings drift up to 1.4e-5 from it on
// 1280-wide rows, one fma stays within 1.2e-7), i0 = int(src), i1 = i0 + (i0 < in - 1), lambda = src - i0, and the
// blend (1-ly) * ((1-lx) * a + lx * b) + ly * ((1-lx) * c + lx * d) with every product and sum rounded.
//
// One thread per four consecutive output columns of one (plane, row): a 16-byte store where the row pitch and the
// base allow it (always so for the session's staging buffers: wp is a multiple of the stride 32), scalar stores
// otherwise.  The eight source texels of a lane sit in two source rows, next to its neighbours': the loads of a
// wave cover two contiguous row segments.  HBM-bound: at ratio r each output texel reads ~1/r^2 source texels once.
#include <cmath>

#include "common.hpp"

#pragma clang fp contract(off)

namespace ydbl {

constexpr int SI_THREADS = 256;

struct ScaleImgArgs {
  const float* x;
  float* y;
  int h, w, sh, sw, hp, wp, flip;
  float sy, sx;  // float(in) / float(out) per axis
  float pad;
};

// source taps of destination index d: (i0, i1, lambda)
__device__ __forceinline__ void si_tap(int d, float scale, int in, int& i0, int& i1, float& l) {
  const float s = fmaxf(__builtin_fmaf(scale, float(d) + 0.5f, -0.5f), 0.f);
  i0 = min((int)s, in - 1);
  i1 = min(i0 + 1, in - 1);
  l = fminf(fmaxf(s - float(i0), 0.f), 1.f);
}

template <bool VEC>
__global__ __launch_bounds__(SI_THREADS) void scale_img_kernel(ScaleImgArgs p) {
  const int plane = blockIdx.z, oy = blockIdx.y;
  const int ox0 = (blockIdx.x * SI_THREADS + threadIdx.x) * 4;
  if (ox0 >= p.wp) return;
  float v[4] = {p.pad, p.pad, p.pad, p.pad};
  if (oy < p.sh && ox0 < p.sw) {
    int y0, y1;
    float ly;
    si_tap(oy, p.sy, p.h, y0, y1, ly);
    const float* r0 = p.x + ((int64_t)plane * p.h + y0) * p.w;
    const float* r1 = p.x + ((int64_t)plane * p.h + y1) * p.w;
    const float wy0 = 1.f - ly;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ox = ox0 + k;
      if (ox < p.sw) {
        int x0, x1;
        float lx;
        si_tap(ox, p.sx, p.w, x0, x1, lx);
        if (p.flip) {  // texel i of x.flip(3) is texel w - 1 - i of x
          x0 = p.w - 1 - x0;
          x1 = p.w - 1 - x1;
        }
        const float wx0 = 1.f - lx;
        const float top = wx0 * r0[x0] + lx * r0[x1];
        const float bot = wx0 * r1[x0] + lx * r1[x1];
        v[k] = wy0 * top + ly * bot;
      }
    }
  }
  float* o = p.y + ((int64_t)plane * p.hp + oy) * p.wp + ox0;
  if constexpr (VEC) {
    *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ox0 + k < p.wp) o[k] = v[k];
  }
}

}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_scale_img(const ydbl_scale_img_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "scale_img: null descriptor");
  if (!d->x || !d->y) return fail(YDBL_EINVAL, "scale_img: null buffer");
  if (d->n < 1 || d->c < 1 || d->h < 1 || d->w < 1 || d->sh < 1 || d->sw < 1 || d->hp < 1 || d->wp < 1)
    return fail(YDBL_EINVAL, "scale_img: extents must be positive");
  if (d->sh > d->hp || d->sw > d->wp) return fail(YDBL_EINVAL, "scale_img: resized extent exceeds the padded output");
  if ((int64_t)d->n * d->c > 65535 || d->hp > 65535) return fail(YDBL_EINVAL, "scale_img: batch / output too large");
  ScaleImgArgs a;
  a.x = d->x; a.y = d->y;
  a.h = d->h; a.w = d->w; a.sh = d->sh; a.sw = d->sw; a.hp = d->hp; a.wp = d->wp;
  a.flip = d->flip ? 1 : 0;
  a.sy = (float)d->h / (float)d->sh;
  a.sx = (float)d->w / (float)d->sw;
  a.pad = d->pad_value;
  dim3 grid((unsigned)cdiv(cdiv(d->wp, 4), SI_THREADS), (unsigned)d->hp, (unsigned)(d->n * d->c));
  hipStream_t s = as_stream(stream);
  if (d->wp % 4 == 0 && reinterpret_cast<uintptr_t>(d->y) % 16 == 0)
    scale_img_kernel<true><<<grid, SI_THREADS, 0, s>>>(a);
  else
    scale_img_kernel<false><<<grid, SI_THREADS, 0, s>>>(a);
  return check_launch("ydbl_scale_img");
}
