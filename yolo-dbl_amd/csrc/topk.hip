// The end2end (YOLOv10) detection tail: ydbl_detect_topk (include/ydbl.h) -- Detect.postprocess's two chained topk's
// (U/nn/modules/head.py:200-221) and the six-column branch of non_max_suppression (U/utils/ops.py:224-228) over the
// multi-label candidate lists of the decode.
//
// Order: (score descending, cand_idx ascending) = ascending 64-bit key (inverted score bits | cand_idx), the key of the
// NMS sort.  Keys are distinct within an image (cand_idx is), so "the first k" is a set and the output is a function
// of the candidate SET: neither the order of the list nor the order in which an atomic lands can show in it.
//
// select  : one 1024-thread workgroup per image.  A radix select over the key's 8-bit digits, most significant first,
//           finds the k-th key: per level a 256-bin LDS histogram of the candidates that match the digits found so
//           far, one wave scans it.  The digits of cand_idx above log2(cap) are skipped, and the select stops at the
//           first level whose bin is taken whole (with distinct scores: after the score's four digits at the latest).
//           The <= k candidates at or below the k-th key are compacted into LDS, ranked there by key (rank = number of
//           smaller keys: k^2 / 1024 broadcast LDS reads per thread, no barrier per stage), filtered by `classes`
//           behind the cut with the gaps closed (ballot prefix), and written with the rows past the count zeroed.
// split   : ahead of it when the lists are long (per_image = 0).  hist: (chunk, image) workgroups count the candidates
//           per score bin (bits >> 19: exponent and four mantissa bits, 4096 bins) in LDS and add their non-empty
//           bins to the image's global histogram -- integer atomics, the sums do not depend on their order.  compact:
//           every workgroup finds the lowest bin a survivor can lie in (the bins above it hold fewer than k
//           candidates) and appends the slots of its candidates in that bin or above to the image's short list, which
//           the select then reads instead of the whole list.  Scores that all share one bin are compacted to the whole
//           list: slower, the same result.
#include "common.hpp"
#include "decode_math.hpp"

namespace ydbl {

constexpr int TK_THREADS = 1024;
constexpr int TK_MAX = 4096;   // max_det limit: the survivors' keys and slots live in LDS (48 KB)
constexpr int TK_BINS = 4096;  // split path: positive fp32 bits >> 19
constexpr int TK_CHUNKS = 128;  // split path: workgroups per image at most

struct TopkArgs {
  const float* cbox; const float* cscore; const int* ccls; const int* cidx; const int* ccount;
  int cap, k, max_det, idx_bits;
  const int* classes; int ncls;
  float clip_w, clip_h;
  float* out; int* out_count;
  int64_t ostride, cstride;
  int* ghist; int* gcount; int* glist;  // split path: [n][TK_BINS], [n], [n][cap]
};

__device__ __forceinline__ uint64_t topk_key(float score, int idx) {
  return ((uint64_t)(0xFFFFFFFFu - __float_as_uint(score)) << 32) | (uint32_t)idx;
}

__device__ __forceinline__ int topk_bin(float score) {
  const uint32_t v = __float_as_uint(score) >> 19;
  return v < (uint32_t)TK_BINS ? (int)v : TK_BINS - 1;  // (a negative score is outside the contract: kept in range)
}

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

__global__ void topk_zero_kernel(int* p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = 0;
}

__global__ __launch_bounds__(256) void topk_hist_kernel(TopkArgs p) {
  __shared__ int h[TK_BINS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = max(min(p.ccount[b], p.cap), 0);
  if ((int64_t)blockIdx.x * 256 >= n) return;  // whole workgroup
  for (int i = tid; i < TK_BINS; i += 256) h[i] = 0;
  __syncthreads();
  const float* sc = p.cscore + (int64_t)b * p.cap;
  for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) atomicAdd(&h[topk_bin(sc[i])], 1);
  __syncthreads();
  int* gh = p.ghist + (int64_t)b * TK_BINS;
  for (int i = tid; i < TK_BINS; i += 256)
    if (h[i]) atomicAdd(&gh[i], h[i]);
}

__global__ __launch_bounds__(256) void topk_compact_kernel(TopkArgs p) {
  __shared__ int wsum[4];
  __shared__ int s_t;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = max(min(p.ccount[b], p.cap), 0);
  if ((int64_t)blockIdx.x * 256 >= n) return;  // whole workgroup
  // the lowest bin that can hold a survivor: the largest t with count(bin >= t) >= k (0 when the image has fewer)
  const int* gh = p.ghist + (int64_t)b * TK_BINS;
  const int top = TK_BINS - 1 - 16 * tid;  // this thread's 16 bins, top downwards
  int loc[16], s = 0;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    loc[q] = gh[top - q];
    s += loc[q];
  }
  int incl = wave_incl_scan(s);
  if (lane == 63) wsum[wave] = incl;
  if (tid == 0) s_t = 0;
  __syncthreads();
  for (int w = 0; w < wave; ++w) incl += wsum[w];
  const int excl = incl - s;
  if (excl < p.k && p.k <= incl) {  // one thread
    int c = excl;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      c += loc[q];
      if (c >= p.k) {
        s_t = top - q;
        break;
      }
    }
  }
  __syncthreads();
  const int t = s_t;
  const float* sc = p.cscore + (int64_t)b * p.cap;
  int* list = p.glist + (int64_t)b * p.cap;
  for (int i0 = blockIdx.x * 256; i0 < n; i0 += gridDim.x * 256) {  // whole waves: wave_slot ballots
    const int i = i0 + tid;
    const bool keep = i < n && topk_bin(sc[i]) >= t;
    const int slot = wave_slot(p.gcount + b, keep);
    if (keep && slot < p.cap) list[slot] = i;
  }
}

__global__ __launch_bounds__(TK_THREADS) void topk_select_kernel(TopkArgs p, int split) {
  __shared__ uint64_t lkey[TK_MAX];
  __shared__ int lslot[TK_MAX];
  __shared__ int hist[256];
  __shared__ int wtot[TK_THREADS / 64];
  __shared__ int s_cnt, s_digit, s_rem, s_done;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* list = split ? p.glist + (int64_t)b * p.cap : nullptr;
  const int n = max(min(split ? p.gcount[b] : p.ccount[b], p.cap), 0);
  const float* sc = p.cscore + (int64_t)b * p.cap;
  const int* ix = p.cidx + (int64_t)b * p.cap;
  const int K = min(p.k, n);
  uint64_t kth = ~0ull;  // every candidate survives when there are at most k
  if (n > K) {           // (uniform: K = k >= 1)
    uint64_t prefix = 0;
    int rem = K;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (shift < 32 && shift >= p.idx_bits) continue;  // cand_idx < 2^idx_bits: this digit is 0 in every key
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const uint64_t hi = shift == 56 ? 0ull : ~0ull << (shift + 8);
      for (int i = tid; i < n; i += TK_THREADS) {
        const int s = list ? list[i] : i;
        const uint64_t key = topk_key(sc[s], ix[s]);
        if (((key ^ prefix) & hi) == 0) atomicAdd(&hist[(int)(key >> shift) & 255], 1);
      }
      __syncthreads();
      if (tid < 64) {  // the digit whose bin holds the rem-th smallest key among the matching ones
        int c[4], s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          c[q] = hist[tid * 4 + q];
          s += c[q];
        }
        const int incl = wave_incl_scan(s);
        int a = incl - s;
        if (a < rem && rem <= incl) {  // one lane
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (a + c[q] >= rem) {
              s_digit = tid * 4 + q;
              s_rem = rem - a;
              s_done = c[q] == rem - a;  // the bin is taken whole: nothing left to split
              break;
            }
            a += c[q];
          }
        }
      }
      __syncthreads();
      prefix |= (uint64_t)s_digit << shift;
      rem = s_rem;
      const int done = s_done;
      __syncthreads();  // s_* and hist are rewritten by the next level
      if (done) {
        if (shift) prefix |= (1ull << shift) - 1;
        break;
      }
    }
    kth = prefix;
  }
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  for (int i = tid; i < n; i += TK_THREADS) {
    const int s = list ? list[i] : i;
    const uint64_t key = topk_key(sc[s], ix[s]);
    if (key <= kth) {
      const int pos = atomicAdd(&s_cnt, 1);
      if (pos < TK_MAX) {
        lkey[pos] = key;
        lslot[pos] = s;
      }
    }
  }
  __syncthreads();
  const int M = min(s_cnt, TK_MAX);  // = K (more only if keys repeat, which the contract excludes)
  // rank by key; the LDS position (arbitrary) orders nothing but repeated keys
  int rk[TK_MAX / TK_THREADS], sl[TK_MAX / TK_THREADS];
#pragma unroll
  for (int q = 0; q < TK_MAX / TK_THREADS; ++q) {
    const int e = tid + q * TK_THREADS;
    rk[q] = TK_MAX;
    sl[q] = 0;
    if (e < M) {
      const uint64_t key = lkey[e];
      int r = 0;
      for (int j = 0; j < M; ++j) {
        const uint64_t kj = lkey[j];
        r += (kj < key || (kj == key && j < e)) ? 1 : 0;
      }
      rk[q] = r;
      sl[q] = lslot[e];
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < TK_MAX / TK_THREADS; ++q)
    if (rk[q] < TK_MAX) lslot[rk[q]] = sl[q];
  __syncthreads();
  // the `classes` filter behind the cut, gaps closed, order kept; then the rows past the count
  const int kout = min(M, K);
  float* out = p.out + (int64_t)b * p.ostride;
  int base = 0;
  for (int r0 = 0; r0 < kout; r0 += TK_THREADS) {
    const int r = r0 + tid;
    bool keep = false;
    int s = 0, c = 0;
    if (r < kout) {
      s = lslot[r];
      c = p.ccls[(int64_t)b * p.cap + s];
      keep = class_ok(c, p.classes, p.ncls);
    }
    const uint64_t m = __ballot(keep);
    if (lane == 0) wtot[wave] = __popcll(m);
    __syncthreads();
    int off = base, tot = 0;
    for (int w = 0; w < TK_THREADS / 64; ++w) {
      if (w < wave) off += wtot[w];
      tot += wtot[w];
    }
    if (keep) {
      const int row = off + __popcll(m & ((1ull << lane) - 1));
      const int64_t o = (int64_t)b * p.cap + s;
      f32x4 v = *reinterpret_cast<const f32x4*>(p.cbox + o * 4);
      if (p.clip_w > 0.f) {
        v[0] = fminf(fmaxf(v[0], 0.f), p.clip_w);
        v[2] = fminf(fmaxf(v[2], 0.f), p.clip_w);
      }
      if (p.clip_h > 0.f) {
        v[1] = fminf(fmaxf(v[1], 0.f), p.clip_h);
        v[3] = fminf(fmaxf(v[3], 0.f), p.clip_h);
      }
      float* d = out + (int64_t)row * 6;
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
      d[4] = sc[s];
      d[5] = (float)c;
    }
    base += tot;
    __syncthreads();
  }
  for (int i = base * 6 + tid; i < p.max_det * 6; i += TK_THREADS) out[i] = 0.f;
  if (tid == 0) p.out_count[(int64_t)b * p.cstride] = base;
}

// [histograms n x TK_BINS int][short-list counts n int, padded to 16 B][short lists n x cap int]
static int64_t topk_counts_bytes(int32_t n) { return ((int64_t)n * 4 + 15) / 16 * 16; }

}  // namespace ydbl

using namespace ydbl;

extern "C" int64_t ydbl_detect_topk_workspace(int32_t n, int32_t cap) {
  if (n < 1 || cap < 1) return 16;
  return (int64_t)n * TK_BINS * 4 + topk_counts_bytes(n) + (int64_t)n * cap * 4;
}

extern "C" int ydbl_detect_topk(const ydbl_topk_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "topk: null descriptor");
  if (!d->cand_box || !d->cand_score || !d->cand_cls || !d->cand_idx || !d->cand_count || !d->out || !d->out_count)
    return fail(YDBL_EINVAL, "topk: null buffer");
  if (d->n < 1 || d->cap < 1) return fail(YDBL_EINVAL, "topk: empty batch");
  if (d->n > 65535) return fail(YDBL_EINVAL, "topk: n <= 65535");
  if (d->max_det < 1 || d->max_det > TK_MAX) return fail(YDBL_EINVAL, "topk: max_det must be in [1, 4096]");
  if (d->k_head < 1) return fail(YDBL_EINVAL, "topk: k_head must be >= 1");
  if (d->nclasses < 0 || (d->classes && d->nclasses < 1) || (!d->classes && d->nclasses))
    return fail(YDBL_EINVAL, "topk: classes / nclasses disagree");
  if (d->out_stride < 0 || (d->out_stride && d->out_stride < (int64_t)d->max_det * 6) || d->count_stride < 0)
    return fail(YDBL_EINVAL, "topk: out_stride must be 0 or >= max_det * 6, count_stride >= 0");
  if (!d->per_image && (!d->workspace || d->workspace_bytes < ydbl_detect_topk_workspace(d->n, d->cap)))
    return fail(YDBL_EINVAL, "topk: workspace below ydbl_detect_topk_workspace(n, cap)");
  hipStream_t s = as_stream(stream);
  TopkArgs a{};
  a.cbox = d->cand_box; a.cscore = d->cand_score; a.ccls = d->cand_cls; a.cidx = d->cand_idx;
  a.ccount = d->cand_count;
  a.cap = d->cap;
  a.k = std::min(d->k_head, d->max_det);
  a.max_det = d->max_det;
  a.idx_bits = 1;
  while (a.idx_bits < 32 && (1ll << a.idx_bits) < (int64_t)d->cap) ++a.idx_bits;  // cand_idx < cap
  a.classes = d->classes; a.ncls = d->nclasses;
  a.clip_w = d->clip_w; a.clip_h = d->clip_h;
  a.out = d->out; a.out_count = d->out_count;
  a.ostride = d->out_stride ? d->out_stride : (int64_t)d->max_det * 6;
  a.cstride = d->count_stride ? d->count_stride : 1;
  if (!d->per_image) {
    a.ghist = reinterpret_cast<int*>(d->workspace);
    a.gcount = a.ghist + (int64_t)d->n * TK_BINS;
    a.glist = reinterpret_cast<int*>(reinterpret_cast<char*>(a.gcount) + topk_counts_bytes(d->n));
    const int64_t words = (int64_t)d->n * TK_BINS + topk_counts_bytes(d->n) / 4;
    topk_zero_kernel<<<(unsigned)std::min<int64_t>(cdiv(words, 256), 1024), 256, 0, s>>>(a.ghist, words);
    const dim3 grid((unsigned)std::min<int64_t>(cdiv(d->cap, 256 * 8), TK_CHUNKS), (unsigned)d->n);
    topk_hist_kernel<<<grid, 256, 0, s>>>(a);
    topk_compact_kernel<<<grid, 256, 0, s>>>(a);
  }
  topk_select_kernel<<<d->n, TK_THREADS, 0, s>>>(a, d->per_image ? 0 : 1);
  return check_launch("ydbl_detect_topk");
}
