// COCO-protocol box matching of NMS detections to ground-truth labels on the device: the per-image, per-category
// evaluation of the COCO detection protocol (COCOeval.evaluateImg as the reference's val() reaches it with
// save_json on a COCO-layout dataset, models/yolo/detect/val.py:297-337), without crowd labels.
//
// One workgroup per (category k, image b); a pair without detections has nothing to write and exits once its rows and
// labels are counted.
//   1. The image's rows of class k are ranked by score descending, ties in row order (a stable sort, as a count of
//      the rows that precede each one), and the first max_dets of them are staged in LDS in rank order as fp64
//      x, y, w, h.  The labels of class k are compacted into LDS in label order by wave 0 (ballot prefix).
//   2. Wave w runs the greedy sequences of the area ranges w, w + 4, ...: detections in rank order, thresholds
//      inside, lanes over the labels.  A lane keeps, for its labels, a T-bit "taken" word per label (its first
//      label's in a register, the rest in LDS where only the owning lane ever touches them) and offers its best
//      candidate; when any lane offers one, a wave-wide arg-max on
//      (non-ignored before ignored, IoU, position in label order) picks the label: the protocol's scan keeps a
//      running best and skips only on iou < best, so on an exact tie the later label wins, and it leaves the
//      non-ignored group only when that group offered nothing.
// The block of category 0 also owns the image-wide outputs: the label ignore flags, the rows that belong to no
// category (rank -1) and their count.  Every output word is written by exactly one thread with a plain vector store,
// so the result does not depend on scheduling.
// IoU, areas and every compare are fp64 in the protocol's operation order with contraction off (pragma below).
#include "common.hpp"

#pragma clang fp contract(off)

namespace ydbl {
namespace {

constexpr int CE_THREADS = 256;
constexpr int CE_WAVES = CE_THREADS / 64;
constexpr int CE_MAX_T = 16;
constexpr int CE_MAX_A = 8;
constexpr int CE_MAX_CUT = 1024;
constexpr int CE_MAX_NC = 32767;  // gridDim.x; n goes to gridDim.y (<= 65535)
constexpr int64_t CE_LDS_LIMIT = 160 * 1024;

struct CocoArgs {
  const float* det; const int* det_count;
  int n, max_det;
  const float* gt_box; const float* gt_cls; const int* gt_ofs;
  int n_gt, single_cls, nc, n_thr, n_area, cut;
  int gcap;  // labels the LDS carve holds (n_gt)
  double thr[CE_MAX_T];
  double area[CE_MAX_A][2];
  int* dt_rank; int* dt_matched; int* dt_ignored; uint8_t* gt_ignore; int* invalid;
};

// the class index of a row or label as the confusion matrix takes it: truncation, -1 outside [0, nc)
__device__ __forceinline__ int ce_cls(float c, int nc) { return c > -1.0f && c < (float)nc ? (int)c : -1; }
// a score for ordering: NaN sorts last
__device__ __forceinline__ float ce_score(float s) { return s == s ? s : -INFINITY; }

// the protocol's IoU of two x, y, w, h boxes
__device__ __forceinline__ double ce_iou(double dx, double dy, double dw, double dh, double gx, double gy, double gw,
                                         double gh) {
  const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
  const double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
  if (iw <= 0.0 || ih <= 0.0) return 0.0;
  const double i = iw * ih;
  return i / (dw * dh + gw * gh - i);
}
// a label's group for one area range: 2 = counted (scanned first), 1 = ignored
__device__ __forceinline__ int ce_group(double area, double a0, double a1) { return area < a0 || area > a1 ? 1 : 2; }

// dynamic LDS: doubles first.  dbox [cut][4] | gbox [gcap][4] | drow int [cut] | taken u32 [CE_WAVES][gcap]
__host__ __device__ inline int64_t ce_lds_bytes(int cut, int gcap) {
  return 32 * (int64_t)cut + 32 * (int64_t)gcap + 4 * (int64_t)cut + 4 * (int64_t)CE_WAVES * gcap;
}

__global__ __launch_bounds__(CE_THREADS) void coco_match_kernel(CocoArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ce_lds[];
  __shared__ int s_m, s_bad, s_g;
  double* dbox = reinterpret_cast<double*>(ce_lds);
  double* gbox = dbox + 4 * (int64_t)p.cut;
  int* drow = reinterpret_cast<int*>(gbox + 4 * (int64_t)p.gcap);
  unsigned* taken = reinterpret_cast<unsigned*>(drow + p.cut);

  const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = wave_id();
  const int g0 = min(max(p.gt_ofs[b], 0), p.n_gt);
  const int nl = min(max(p.gt_ofs[b + 1], g0), p.n_gt) - g0;
  const int nd = max(min(p.det_count[b], p.max_det), 0);
  const float* det = p.det + (int64_t)b * p.max_det * 6;
  const int64_t row0 = (int64_t)b * p.max_det;
  const int A = p.n_area, T = p.n_thr;

  if (tid == 0) { s_m = 0; s_bad = 0; s_g = 0; }
  __syncthreads();

  // ---- the image-wide outputs (category 0's block) ----
  if (k == 0) {
    int bad = 0;
    for (int d = tid; d < p.max_det; d += CE_THREADS) {
      const bool none = d >= nd || (!p.single_cls && ce_cls(det[d * 6 + 5], p.nc) < 0);
      if (!none) continue;
      bad += d < nd;
      p.dt_rank[row0 + d] = -1;
      for (int a = 0; a < A; ++a) { p.dt_matched[(row0 + d) * A + a] = 0; p.dt_ignored[(row0 + d) * A + a] = 0; }
    }
    if (bad) atomicAdd(&s_bad, bad);
    for (int l = tid; l < nl; l += CE_THREADS) {
      const float* g = p.gt_box + (int64_t)(g0 + l) * 4;
      const double ar = ((double)g[2] - (double)g[0]) * ((double)g[3] - (double)g[1]);
      for (int a = 0; a < A; ++a) p.gt_ignore[(int64_t)(g0 + l) * A + a] = ar < p.area[a][0] || ar > p.area[a][1];
    }
  }

  // ---- rank the rows of class k, stage the first `cut` ----
  int mine = 0;
  for (int d = tid; d < nd; d += CE_THREADS) {
    const int c = p.single_cls ? 0 : ce_cls(det[d * 6 + 5], p.nc);
    if (c != k) continue;
    ++mine;
    const float s = ce_score(det[d * 6 + 4]);
    int rank = 0;
    for (int j = 0; j < nd; ++j) {
      const int cj = p.single_cls ? 0 : ce_cls(det[j * 6 + 5], p.nc);
      const float sj = ce_score(det[j * 6 + 4]);
      rank += cj == k && (sj > s || (sj == s && j < d));
    }
    if (rank < p.cut) {
      const double x = det[d * 6], y = det[d * 6 + 1];
      dbox[rank * 4] = x; dbox[rank * 4 + 1] = y;
      dbox[rank * 4 + 2] = (double)det[d * 6 + 2] - x; dbox[rank * 4 + 3] = (double)det[d * 6 + 3] - y;
      drow[rank] = d;
      p.dt_rank[row0 + d] = rank;
    } else {
      p.dt_rank[row0 + d] = -1;
      for (int a = 0; a < A; ++a) { p.dt_matched[(row0 + d) * A + a] = 0; p.dt_ignored[(row0 + d) * A + a] = 0; }
    }
  }
  if (mine) atomicAdd(&s_m, mine);

  // ---- the labels of class k, in label order (wave 0) ----
  if (wave == 0) {
    int run = 0;
    for (int l0 = 0; l0 < nl; l0 += 64) {
      const int l = l0 + lane;
      const bool hit = l < nl && (p.single_cls ? 0 : ce_cls(p.gt_cls[g0 + l], p.nc)) == k;
      const unsigned long long bal = __ballot(hit);
      if (hit) {
        const int pos = run + __popcll(bal & ((1ull << lane) - 1));
        const float* g = p.gt_box + (int64_t)(g0 + l) * 4;
        const double x = g[0], y = g[1];
        gbox[pos * 4] = x; gbox[pos * 4 + 1] = y;
        gbox[pos * 4 + 2] = (double)g[2] - x; gbox[pos * 4 + 3] = (double)g[3] - y;
      }
      run += __popcll(bal);
    }
    if (lane == 0) s_g = run;
  }
  __syncthreads();
  if (k == 0 && tid == 0) p.invalid[b] = s_bad;
  const int D = min(s_m, p.cut), G = s_g;  // G <= nl <= n_gt == gcap
  if (D == 0) return;

  // ---- the greedy sequences: one area range per wave at a time ----
  // A lane's first label (index `lane`) keeps its IoU with the current detection, its group and its taken word in
  // registers across the thresholds; labels past the wave width are re-evaluated per threshold from LDS.
  unsigned* tk = taken + (int64_t)wave * p.gcap;
  for (int a = wave; a < A; a += CE_WAVES) {
    const double a0 = p.area[a][0], a1 = p.area[a][1];
    for (int l = lane + 64; l < G; l += 64) tk[l] = 0;
    unsigned tk0 = 0;
    double g0x = 0, g0y = 0, g0w = 0, g0h = 0;
    if (lane < G) { g0x = gbox[lane * 4]; g0y = gbox[lane * 4 + 1]; g0w = gbox[lane * 4 + 2]; g0h = gbox[lane * 4 + 3]; }
    const int pl0 = lane < G ? ce_group(g0w * g0h, a0, a1) : 0;
    for (int r = 0; r < D; ++r) {
      const double dx = dbox[r * 4], dy = dbox[r * 4 + 1], dw = dbox[r * 4 + 2], dh = dbox[r * 4 + 3];
      const double darea = dw * dh;
      const bool dout = darea < a0 || darea > a1;
      const double v0 = lane < G ? ce_iou(dx, dy, dw, dh, g0x, g0y, g0w, g0h) : 0.0;
      unsigned mm = 0, mi = 0;
      for (int t = 0; t < T; ++t) {
        const double thr = p.thr[t];
        int pri = 0, bl = -1;
        double bv = 0.0;
        if (pl0 && !((tk0 >> t) & 1) && v0 >= thr) { pri = pl0; bv = v0; bl = lane; }
        for (int l = lane + 64; l < G; l += 64) {
          if ((tk[l] >> t) & 1) continue;
          const double gw = gbox[l * 4 + 2], gh = gbox[l * 4 + 3];
          const double v = ce_iou(dx, dy, dw, dh, gbox[l * 4], gbox[l * 4 + 1], gw, gh);
          if (!(v >= thr)) continue;
          const int pl = ce_group(gw * gh, a0, a1);
          if (pl > pri || (pl == pri && v >= bv)) { pri = pl; bv = v; bl = l; }  // l ascends: a tie takes the later
        }
        if (__ballot(pri > 0)) {  // wave-uniform: some lane offers a label
          for (int o = 32; o > 0; o >>= 1) {
            const int op = __shfl_xor(pri, o), ol = __shfl_xor(bl, o);
            const double ov = __shfl_xor(bv, o);
            if (op > pri || (op == pri && (ov > bv || (ov == bv && ol > bl)))) { pri = op; bv = ov; bl = ol; }
          }
          mm |= 1u << t;
          if (pri == 1) mi |= 1u << t;
          if (bl == lane) tk0 |= 1u << t;
          else if ((bl & 63) == lane) tk[bl] |= 1u << t;  // the owning lane
        } else if (dout) {
          mi |= 1u << t;
        }
      }
      if (lane == 0) {
        const int64_t o = (row0 + drow[r]) * A + a;
        p.dt_matched[o] = (int)mm;
        p.dt_ignored[o] = (int)mi;
      }
    }
  }
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int64_t ydbl_coco_workspace(int32_t n, int32_t max_det, int32_t n_gt, int32_t nc) {
  if (n < 0 || max_det < 0 || n_gt < 0 || nc < 0) return -1;
  return 0;  // the matching state lives in LDS
}

extern "C" int ydbl_coco_match(const ydbl_coco_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "coco_match: null descriptor");
  if (!d->det || !d->det_count || !d->gt_ofs || !d->iou_thrs || !d->area_rng || !d->dt_rank || !d->dt_matched ||
      !d->dt_ignored || !d->invalid)
    return fail(YDBL_EINVAL, "coco_match: null buffer");
  if (d->n < 1 || d->max_det < 1) return fail(YDBL_EINVAL, "coco_match: empty batch");
  if (d->n > 65535) return fail(YDBL_EINVAL, "coco_match: n must be <= 65535");
  if (d->max_det > (1 << 20)) return fail(YDBL_EINVAL, "coco_match: max_det must be <= 2^20");
  if (d->n_gt < 0 || (d->n_gt > 0 && (!d->gt_box || !d->gt_cls || !d->gt_ignore)))
    return fail(YDBL_EINVAL, "coco_match: labels missing");
  if (d->nc < 1 || d->nc > CE_MAX_NC) return fail(YDBL_EINVAL, "coco_match: nc must be in [1, 32767]");
  if (d->n_iou < 1 || d->n_iou > CE_MAX_T) return fail(YDBL_EINVAL, "coco_match: n_iou must be in [1, 16]");
  if (d->n_area < 1 || d->n_area > CE_MAX_A) return fail(YDBL_EINVAL, "coco_match: n_area must be in [1, 8]");
  if (d->max_dets < 1 || d->max_dets > CE_MAX_CUT)
    return fail(YDBL_EINVAL, "coco_match: max_dets must be in [1, 1024]");
  if (ydbl_coco_workspace(d->n, d->max_det, d->n_gt, d->nc) > 0 && !d->workspace)
    return fail(YDBL_EINVAL, "coco_match: workspace missing");
  CocoArgs a;
  for (int t = 0; t < d->n_iou; ++t) {
    if (!(d->iou_thrs[t] == d->iou_thrs[t])) return fail(YDBL_EINVAL, "coco_match: a NaN IoU threshold");
    a.thr[t] = d->iou_thrs[t] < 1 - 1e-10 ? d->iou_thrs[t] : 1 - 1e-10;  // min(t, 1 - 1e-10)
  }
  for (int r = 0; r < d->n_area; ++r) {
    a.area[r][0] = d->area_rng[2 * r]; a.area[r][1] = d->area_rng[2 * r + 1];
    if (!(a.area[r][0] <= a.area[r][1])) return fail(YDBL_EINVAL, "coco_match: an area range with lo > hi or NaN");
  }
  const int cut = d->max_dets < d->max_det ? d->max_dets : d->max_det;
  const int64_t lds = ce_lds_bytes(cut, d->n_gt);
  if (lds + 64 > CE_LDS_LIMIT)
    return fail(YDBL_ECAPACITY, "coco_match: " + std::to_string(cut) + " detections and " + std::to_string(d->n_gt) +
                                    " labels need " + std::to_string(lds) +
                                    " bytes of LDS, more than the 160 KiB of a workgroup");
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(coco_match_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(YDBL_ELAUNCH, std::string("coco_match: ") + hipGetErrorString(e));
  }
  a.det = d->det; a.det_count = d->det_count; a.n = d->n; a.max_det = d->max_det;
  a.gt_box = d->gt_box; a.gt_cls = d->gt_cls; a.gt_ofs = d->gt_ofs; a.n_gt = d->n_gt;
  a.single_cls = d->single_cls != 0; a.nc = d->nc; a.n_thr = d->n_iou; a.n_area = d->n_area; a.cut = cut;
  a.gcap = d->n_gt;
  a.dt_rank = d->dt_rank; a.dt_matched = d->dt_matched; a.dt_ignored = d->dt_ignored;
  a.gt_ignore = d->gt_ignore; a.invalid = d->invalid;
  coco_match_kernel<<<dim3(d->nc, d->n), CE_THREADS, (size_t)lds, as_stream(stream)>>>(a);
  return check_launch("ydbl_coco_match");
}
