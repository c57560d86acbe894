// Mask side of segmentation validation on bit planes, gfx950: SegmentationValidator._process_batch(masks=True)
// (U/models/yolo/segment/val.py:204-213) up to the IoU matrix; the matching itself is match_kernel (val.hip).
//
// The reference builds fp32 [n, H, W] planes for the labels (torch.where(gt_masks == index, 1.0, 0.0), bilinear
// resampling to the prediction's size, > 0.5) and multiplies them against the fp32 prediction planes (mask_iou,
// U/utils/metrics.py:137-153).  Both are 0 / 1, so here they are bit planes -- 64 pixels to a uint64 word, the layout
// ydbl_process_mask writes with YDBL_MASK_BITS -- and the products are popcount(AND).  The counts are integers below
// 2^24, which fp32 holds exactly, so the IoU is bitwise the reference's.
//
// gt_bits_kernel: one 256-thread workgroup per label.  A wave walks the (row, word) pairs of the plane, lane j
// evaluates pixel 64 q + j and the word is the wave's ballot; the area is the popcount of the ballots, summed over the
// four waves through LDS.  Bilinear by torch's upsample_bilinear2d rule as in mask.hip, each operation rounded alone.
//
// mask_iou_kernel: one 256-thread workgroup per (slot, image).  The detection's plane is staged in LDS a chunk of
// IOU_CHUNK words at a time; wave w takes the labels l = w (mod 4) of the image, its lanes stride the chunk with
// popcount(det & gt) on ground-truth words read through L2, and a shuffle reduction gives the wave the sum.  A
// label's running count over the chunks lives in one lane's register (label k of the wave in lane k), so a pass
// covers 256 labels; more labels take further passes.  No atomics anywhere: every output element has one writer.
#include "common.hpp"

#pragma clang fp contract(off)

namespace ydbl {
namespace {

constexpr int SV_THREADS = 256;
constexpr int IOU_CHUNK = 4096;  // detection words staged per pass (32 KiB)
using u64 = unsigned long long;

struct GtBitsArgs {
  const uint8_t* src; int n, gh, gw, overlap;
  const int* gt_ofs; int n_gt;
  int H, W, wpr;
  u64* bits; int* area;
};

// torch's area_pixel_compute_source_index (align_corners=False), as mk_src of mask.hip
__device__ __forceinline__ float sv_src(float scale, int d) {
  const float t = scale * (float(d) + 0.5f);
  const float s = t - 0.5f;
  return s < 0.f ? 0.f : s;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(SV_THREADS) void gt_bits_kernel(GtBitsArgs a) {
  __shared__ int s_area[SV_THREADS / 64];
  const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the image that owns label g: the last b with gt_ofs[b] <= g
  int lo = 0, hi = a.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.gt_ofs[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const int l = g - a.gt_ofs[lo];
  const uint8_t* src = a.src + (int64_t)(a.overlap ? lo : g) * a.gh * a.gw;
  const int want = l + 1;  // overlap: the value that names this label (one past 255 names nothing)
  auto ind = [&](int i, int j) -> float {
    const int v = src[(int64_t)i * a.gw + j];
    return (a.overlap ? v == want : v != 0) ? 1.f : 0.f;
  };
  const bool same = a.gh == a.H && a.gw == a.W;
  const float sch = float(a.gh) / float(a.H), scw = float(a.gw) / float(a.W);
  u64* plane = a.bits + (int64_t)g * a.H * a.wpr;
  const int words = a.H * a.wpr;
  int area = 0;
  for (int w = wave; w < words; w += SV_THREADS / 64) {  // uniform over the wave
    const int y = w / a.wpr, q = w - y * a.wpr;
    const int x = q * 64 + lane;
    bool on = false;
    if (x < a.W) {
      if (same) {
        on = ind(y, x) != 0.f;
      } else {
        const float syr = sv_src(sch, y), sxr = sv_src(scw, x);
        const int i0 = min(int(syr), a.gh - 1), i1 = min(i0 + 1, a.gh - 1);
        const int j0 = min(int(sxr), a.gw - 1), j1 = min(j0 + 1, a.gw - 1);
        const float h1 = syr - float(i0), h0 = 1.f - h1, w1 = sxr - float(j0), w0 = 1.f - w1;
        const float v = h0 * (w0 * ind(i0, j0) + w1 * ind(i0, j1)) + h1 * (w0 * ind(i1, j0) + w1 * ind(i1, j1));
        on = v > 0.5f;
      }
    }
    const u64 word = __ballot(on);
    if (lane == 0) plane[w] = word;
    area += __popcll(word);
  }
  if (lane == 0) s_area[wave] = area;
  __syncthreads();
  if (threadIdx.x == 0) a.area[g] = s_area[0] + s_area[1] + s_area[2] + s_area[3];
}

struct MaskIouArgs {
  const u64* det; const int64_t* row_offset; const int* count; int n, max_det;
  const u64* gt; const int* gt_ofs; const int* area_gt; int n_gt;
  int words;
  float* iou; int* inter; int* area_det;
};

__global__ __launch_bounds__(SV_THREADS) void mask_iou_kernel(MaskIouArgs a) {
  __shared__ u64 s_det[IOU_CHUNK];
  __shared__ int s_part[SV_THREADS / 64];
  const int d = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g0 = min(max(a.gt_ofs[b], 0), a.n_gt);
  const int nl = min(max(a.gt_ofs[b + 1], g0), a.n_gt) - g0;
  if (d >= min(a.count[b], a.max_det)) {  // no detection in this slot: its column of the image's labels is 0
    for (int l = tid; l < nl; l += SV_THREADS) {
      a.iou[(int64_t)(g0 + l) * a.max_det + d] = 0.f;
      if (a.inter) a.inter[(int64_t)(g0 + l) * a.max_det + d] = 0;
    }
    if (tid == 0 && a.area_det) a.area_det[(int64_t)b * a.max_det + d] = 0;
    return;
  }
  const u64* det = a.det + (a.row_offset[b] + d) * (int64_t)a.words;

  int part = 0;
  for (int w = tid; w < a.words; w += SV_THREADS) part += __popcll(det[w]);
  part = wave_sum(part);
  if (lane == 0) s_part[wave] = part;
  __syncthreads();
  const int area_d = s_part[0] + s_part[1] + s_part[2] + s_part[3];
  if (tid == 0 && a.area_det) a.area_det[(int64_t)b * a.max_det + d] = area_d;

  for (int lg = 0; lg < nl; lg += SV_THREADS) {  // 256 labels a pass: wave w's k-th label is lg + w + 4 k, kept by lane k
    int acc = 0;
    for (int c0 = 0; c0 < a.words; c0 += IOU_CHUNK) {
      const int cw = min(IOU_CHUNK, a.words - c0);
      __syncthreads();  // the previous chunk is consumed
      for (int w = tid; w < cw; w += SV_THREADS) s_det[w] = det[c0 + w];
      __syncthreads();
      for (int k = 0; k < 64; ++k) {
        const int l = lg + wave + 4 * k;  // uniform over the wave
        if (l >= nl) break;
        const u64* gt = a.gt + (int64_t)(g0 + l) * a.words + c0;
        int s = 0;
        for (int w = lane; w < cw; w += 64) s += __popcll(s_det[w] & gt[w]);
        s = wave_sum(s);
        if (lane == k) acc += s;
      }
    }
    const int l = lg + wave + 4 * lane;
    if (l < nl) {
      const float fi = float(acc), fg = float(a.area_gt[g0 + l]), fd = float(area_d);
      a.iou[(int64_t)(g0 + l) * a.max_det + d] = fi / (((fg + fd) - fi) + 1e-7f);
      if (a.inter) a.inter[(int64_t)(g0 + l) * a.max_det + d] = acc;
    }
  }
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int ydbl_gt_mask_bits(const ydbl_gt_bits_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "gt_mask_bits: null descriptor");
  if (d->n < 1 || d->n_gt < 0) return fail(YDBL_EINVAL, "gt_mask_bits: empty batch");
  if (!d->gt_ofs) return fail(YDBL_EINVAL, "gt_mask_bits: null buffer");
  if (d->n_gt == 0) return YDBL_OK;
  if (!d->src || !d->bits || !d->area) return fail(YDBL_EINVAL, "gt_mask_bits: null buffer");
  if (d->gh < 1 || d->gw < 1 || d->out_h < 1 || d->out_w < 1) return fail(YDBL_EINVAL, "gt_mask_bits: empty map");
  if ((int64_t)d->gh * d->gw > (int64_t)1 << 24 || (int64_t)d->out_h * d->out_w > (int64_t)1 << 24)
    return fail(YDBL_EINVAL, "gt_mask_bits: a map of more than 2^24 pixels");
  if (reinterpret_cast<uintptr_t>(d->bits) % 8) return fail(YDBL_EINVAL, "gt_mask_bits: bits must be 8-byte aligned");
  GtBitsArgs a;
  a.src = d->src; a.n = d->n; a.gh = d->gh; a.gw = d->gw; a.overlap = d->overlap != 0;
  a.gt_ofs = d->gt_ofs; a.n_gt = d->n_gt;
  a.H = d->out_h; a.W = d->out_w; a.wpr = (int)cdiv(d->out_w, 64);
  a.bits = reinterpret_cast<u64*>(d->bits); a.area = d->area;
  gt_bits_kernel<<<d->n_gt, SV_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch("ydbl_gt_mask_bits");
}

extern "C" int ydbl_mask_iou(const ydbl_mask_iou_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "mask_iou: null descriptor");
  if (!d->det_bits || !d->row_offset || !d->count || !d->gt_ofs || !d->iou)
    return fail(YDBL_EINVAL, "mask_iou: null buffer");
  if (d->n < 1 || d->n > 65535 || d->max_det < 1) return fail(YDBL_EINVAL, "mask_iou: n must be in [1, 65535], max_det >= 1");
  if (d->n_gt < 0 || (d->n_gt > 0 && (!d->gt_bits || !d->area_gt)))
    return fail(YDBL_EINVAL, "mask_iou: null buffer (labels missing)");
  if (d->out_h < 1 || d->out_w < 1) return fail(YDBL_EINVAL, "mask_iou: empty planes");
  if ((int64_t)d->out_h * d->out_w > (int64_t)1 << 24)
    return fail(YDBL_EINVAL, "mask_iou: out_h * out_w must be <= 2^24 (fp32-exact counts)");
  if (reinterpret_cast<uintptr_t>(d->det_bits) % 8 || reinterpret_cast<uintptr_t>(d->gt_bits) % 8)
    return fail(YDBL_EINVAL, "mask_iou: bit planes must be 8-byte aligned");
  MaskIouArgs a;
  a.det = reinterpret_cast<const u64*>(d->det_bits); a.row_offset = d->row_offset; a.count = d->count;
  a.n = d->n; a.max_det = d->max_det;
  a.gt = reinterpret_cast<const u64*>(d->gt_bits); a.gt_ofs = d->gt_ofs; a.area_gt = d->area_gt; a.n_gt = d->n_gt;
  a.words = d->out_h * (int)cdiv(d->out_w, 64);
  a.iou = d->iou; a.inter = d->inter; a.area_det = d->area_det;
  const dim3 grid((unsigned)d->max_det, (unsigned)d->n);
  mask_iou_kernel<<<grid, SV_THREADS, 0, as_stream(stream)>>>(a);
  return check_launch("ydbl_mask_iou");
}
