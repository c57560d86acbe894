// ByteTrack association on the device (U/trackers/byte_tracker.py:293-405 BYTETracker.update, :51-228 STrack,
// U/trackers/utils/kalman_filter.py:52-236 KalmanFilterXYAH, U/trackers/utils/matching.py:20-157), reading the
// det | count records of ydbl_nms where they lie.  One workgroup per tracker; the tracker's lists live in a
// caller-owned state buffer as unordered slots plus a 64-bit sequence key per slot that reproduces the reference's
// list order (tracked_stracks / lost_stracks: kept tracks keep their place, new and re-found tracks are appended).
//
// Arithmetic: the Kalman filter is fp64 (8x8 products, the 4x4 Cholesky factor and solve); IoU and the fused cost
// are fp32 in numpy's operation order (no contraction: see the pragma below); the assignment runs on those costs
// in fp64 and is exact -- shortest augmenting paths over the real columns plus one implicit zero-cost dummy column
// per row, with edge weight c - thresh and the pairs with c > thresh forbidden, i.e. the minimum of
// sum_matched (c_ij - thresh), which is what lap.lapjv(extend_cost=True, cost_limit=thresh) minimises.  The costs
// are recomputed from the boxes in LDS whenever a row is scanned (about 20 flops) instead of being stored: no
// cost-matrix workspace, no global-memory latency inside the augmenting-path loop.
//
// Every loop is bounded by max_tracks + max_det (or their product) by construction.
#pragma clang fp contract(off)
#include <math.h>

#include "common.hpp"

namespace ydbl {
namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / 64;
enum { ST_FREE = 0, ST_TRACKED = 1, ST_LOST = 2, ST_REMOVED = 3 };
enum { FL_NONE = 0, FL_REFIND = 1, FL_NEWLOST = 2 };
enum { COST_FUSED = 1, COST_IOU = 0 };
constexpr int TK_HEADER_BYTES = 32;  // int64 seq counter | int32 frame_id, next_id, overflow, hwm, 0, 0

struct TrkParams {
  const float* det;
  const int32_t* det_count;
  const float* hw;
  int n, max_det;
  int64_t det_stride, count_stride;
  float high, low, newt;
  double match;
  int fuse, max_time_lost, T, trackers, reset_each;
  float* out;
  int32_t* out_count;
  int32_t* tracked;
  int32_t* out_idx;
  unsigned char* state;
  int64_t state_bytes;
};

// one tracker's slice of the state buffer
struct StateView {
  long long* seqctr;
  int32_t* head;  // frame_id, next_id, overflow, hwm
  double* mean;   // [T][8]
  double* cov;    // [T][64]
  long long* seq; // [T]
  int32_t *state, *act, *id, *frame, *start, *tlen, *idx, *rmem;
  float *score, *cls;
};

__host__ __device__ inline int64_t tk_state_bytes(int T) {
  return (TK_HEADER_BYTES + (int64_t)T * (8 * 8 + 64 * 8 + 8 + 10 * 4) + 15) / 16 * 16;
}

__device__ inline StateView state_view(unsigned char* base, int T) {
  StateView s;
  s.seqctr = reinterpret_cast<long long*>(base);
  s.head = reinterpret_cast<int32_t*>(base + 8);
  s.mean = reinterpret_cast<double*>(base + TK_HEADER_BYTES);
  s.cov = s.mean + (int64_t)T * 8;
  s.seq = reinterpret_cast<long long*>(s.cov + (int64_t)T * 64);
  s.state = reinterpret_cast<int32_t*>(s.seq + T);
  s.act = s.state + T;
  s.id = s.act + T;
  s.frame = s.id + T;
  s.start = s.frame + T;
  s.tlen = s.start + T;
  s.idx = s.tlen + T;
  s.rmem = s.idx + T;
  s.score = reinterpret_cast<float*>(s.rmem + T);
  s.cls = s.score + T;
  return s;
}

// the workgroup's LDS, carved from one dynamic array (doubles first)
struct Lds {
  double *u, *v, *spc;
  long long* tseq;
  float *dtlwh, *dscore, *dcls, *tbox;
  int *dkind, *dused, *collist, *rowlist, *pool, *uncf, *col4row, *tstate, *tact, *tflag, *path, *row4col;
  unsigned char *SR, *SC;
};

__host__ __device__ inline int64_t tk_lds_bytes(int T, int D) {
  const int64_t C = (int64_t)T + D;
  return 8 * (T + 2 * C + T) + 4 * ((int64_t)D * 4 + 2 * D + (int64_t)T * 4 + 3 * D + 7 * (int64_t)T + 2 * C) + T + C + 16;
}

__device__ inline Lds carve(unsigned char* base, int T, int D) {
  const int C = T + D;
  Lds L;
  L.u = reinterpret_cast<double*>(base);
  L.v = L.u + T;
  L.spc = L.v + C;
  L.tseq = reinterpret_cast<long long*>(L.spc + C);
  L.dtlwh = reinterpret_cast<float*>(L.tseq + T);
  L.dscore = L.dtlwh + D * 4;
  L.dcls = L.dscore + D;
  L.tbox = L.dcls + D;
  L.dkind = reinterpret_cast<int*>(L.tbox + T * 4);
  L.dused = L.dkind + D;
  L.collist = L.dused + D;
  L.rowlist = L.collist + D;
  L.pool = L.rowlist + T;
  L.uncf = L.pool + T;
  L.col4row = L.uncf + T;
  L.tstate = L.col4row + T;
  L.tact = L.tstate + T;
  L.tflag = L.tact + T;
  L.path = L.tflag + T;
  L.row4col = L.path + C;
  L.SR = reinterpret_cast<unsigned char*>(L.row4col + C);
  L.SC = L.SR + T;
  return L;
}

struct Shared {
  int frame_id, next_id, overflow, hwm;
  long long seqctr;
  int nd, npool, npt, nuncf, nrows, ncols, nnew, na, nb, nout;
  double red_val[TK_WAVES];
  int red_idx[TK_WAVES];
  int red_free[TK_WAVES];
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }

// bbox_ioa(iou=True) of U/utils/metrics.py:20-49 in fp32, numpy's operation order; a = box1 (x1,y1,x2,y2), b = box2
__device__ __forceinline__ float iou_dist(const float* a, const float* b) {
  float iw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]);
  float ih = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
  iw = iw < 0.0f ? 0.0f : iw;
  ih = ih < 0.0f ? 0.0f : ih;
  const float inter = iw * ih;
  const float area2 = (b[2] - b[0]) * (b[3] - b[1]);
  const float area1 = (a[2] - a[0]) * (a[3] - a[1]);
  const float area = (area2 + area1) - inter;
  const float iou = inter / (area + 1e-7f);
  return 1.0f - iou;
}

// a detection's xyxy as STrack.xyxy gives it from the fp32 _tlwh
__device__ __forceinline__ void det_xyxy(const float* tlwh, float* b) {
  b[0] = tlwh[0];
  b[1] = tlwh[1];
  b[2] = tlwh[2] + tlwh[0];
  b[3] = tlwh[3] + tlwh[1];
}

// STrack.tlwh / .xyxy from the mean, fp64
__device__ __forceinline__ void mean_xyxy(const double* m, double* b) {
  const double w = m[2] * m[3];
  const double x1 = m[0] - w / 2, y1 = m[1] - m[3] / 2;
  b[0] = x1;
  b[1] = y1;
  b[2] = w + x1;
  b[3] = m[3] + y1;
}

__device__ inline void slot_box(const StateView& st, const Lds& L, int s) {
  double b[4];
  mean_xyxy(st.mean + (int64_t)s * 8, b);
  for (int k = 0; k < 4; ++k) L.tbox[s * 4 + k] = (float)b[k];
}

// KalmanFilterXYAH.predict (multi_predict) of one slot, in place; zero_vh: the track is not Tracked (mean[7] = 0)
__device__ inline void kf_predict(const StateView& st, int s, bool zero_vh) {
  double* m = st.mean + (int64_t)s * 8;
  double* Pg = st.cov + (int64_t)s * 64;
  double P[64];
  for (int k = 0; k < 64; ++k) P[k] = Pg[k];
  double m7 = zero_vh ? 0.0 : m[7];
  const double h = m[3];
  const double sp = (1.0 / 20) * h, sv = (1.0 / 160) * h;
  const double q[8] = {sp * sp, sp * sp, 1e-2 * 1e-2, sp * sp, sv * sv, sv * sv, 1e-5 * 1e-5, sv * sv};
  m[0] = m[0] + m[4];
  m[1] = m[1] + m[5];
  m[2] = m[2] + m[6];
  m[3] = h + m7;
  m[7] = m7;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) P[i * 8 + j] += P[(i + 4) * 8 + j];
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) P[i * 8 + j] += P[i * 8 + j + 4];
  for (int i = 0; i < 8; ++i) P[i * 8 + i] += q[i];
  for (int k = 0; k < 64; ++k) Pg[k] = P[k];
}

// KalmanFilterXYAH.update of one slot with the detection's fp32 tlwh (xyah in fp32, as tlwh_to_xyah on _tlwh)
__device__ inline void kf_update(const StateView& st, int s, const float* tlwh) {
  double* m = st.mean + (int64_t)s * 8;
  double* Pg = st.cov + (int64_t)s * 64;
  double P[64];
  for (int k = 0; k < 64; ++k) P[k] = Pg[k];
  const float zx = tlwh[0] + tlwh[2] / 2.0f, zy = tlwh[1] + tlwh[3] / 2.0f, za = tlwh[2] / tlwh[3];
  const double z[4] = {(double)zx, (double)zy, (double)za, (double)tlwh[3]};
  const double sd = (1.0 / 20) * m[3];
  const double r[4] = {sd * sd, sd * sd, 1e-1 * 1e-1, sd * sd};
  double S[16], Lc[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) S[i * 4 + j] = P[i * 8 + j] + (i == j ? r[i] : 0.0);
  for (int k = 0; k < 16; ++k) Lc[k] = 0.0;
  for (int j = 0; j < 4; ++j) {
    double d = S[j * 4 + j];
    for (int k = 0; k < j; ++k) d -= Lc[j * 4 + k] * Lc[j * 4 + k];
    d = sqrt(d);
    Lc[j * 4 + j] = d;
    for (int i = j + 1; i < 4; ++i) {
      double a = S[i * 4 + j];
      for (int k = 0; k < j; ++k) a -= Lc[i * 4 + k] * Lc[j * 4 + k];
      Lc[i * 4 + j] = a / d;
    }
  }
  // K[i][k] = X[k][i], S X = (P H^T)^T, column i of the right-hand side = P[i][0..3]
  double K[32];
  for (int i = 0; i < 8; ++i) {
    double y[4];
    for (int k = 0; k < 4; ++k) {
      double a = P[i * 8 + k];
      for (int l = 0; l < k; ++l) a -= Lc[k * 4 + l] * y[l];
      y[k] = a / Lc[k * 4 + k];
    }
    for (int k = 3; k >= 0; --k) {
      double a = y[k];
      for (int l = k + 1; l < 4; ++l) a -= Lc[l * 4 + k] * K[i * 4 + l];
      K[i * 4 + k] = a / Lc[k * 4 + k];
    }
  }
  double inn[4];
  for (int k = 0; k < 4; ++k) inn[k] = z[k] - m[k];
  for (int i = 0; i < 8; ++i) {
    double a = 0.0;
    for (int k = 0; k < 4; ++k) a += inn[k] * K[i * 4 + k];
    m[i] = m[i] + a;
  }
  double M[32];  // S K^T
  for (int k = 0; k < 4; ++k)
    for (int j = 0; j < 8; ++j) {
      double a = 0.0;
      for (int l = 0; l < 4; ++l) a += S[k * 4 + l] * K[j * 4 + l];
      M[k * 8 + j] = a;
    }
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) {
      double a = 0.0;
      for (int k = 0; k < 4; ++k) a += K[i * 4 + k] * M[k * 8 + j];
      Pg[i * 8 + j] = P[i * 8 + j] - a;
    }
}

// KalmanFilterXYAH.initiate from the detection's fp32 xyah: fp32 roundings of the mean and of the std products
__device__ inline void kf_initiate(const StateView& st, int s, const float* tlwh) {
  double* m = st.mean + (int64_t)s * 8;
  double* Pg = st.cov + (int64_t)s * 64;
  const float zx = tlwh[0] + tlwh[2] / 2.0f, zy = tlwh[1] + tlwh[3] / 2.0f, za = tlwh[2] / tlwh[3], zh = tlwh[3];
  m[0] = zx;
  m[1] = zy;
  m[2] = za;
  m[3] = zh;
  m[4] = m[5] = m[6] = m[7] = 0.0;
  const double sp = (double)((float)(2 * (1.0 / 20)) * zh), sv = (double)((float)(10 * (1.0 / 160)) * zh);
  const double q[8] = {sp * sp, sp * sp, 1e-2 * 1e-2, sp * sp, sv * sv, sv * sv, 1e-5 * 1e-5, sv * sv};
  for (int k = 0; k < 64; ++k) Pg[k] = 0.0;
  for (int i = 0; i < 8; ++i) Pg[i * 8 + i] = q[i];
}

// STrack.update / re_activate of slot s with detection j
__device__ inline void apply_match(const StateView& st, const Lds& L, int s, int j, int fid) {
  kf_update(st, s, L.dtlwh + j * 4);
  if (L.tstate[s] == ST_TRACKED) {
    st.tlen[s] += 1;
  } else {
    st.tlen[s] = 0;
    L.tflag[s] = FL_REFIND;
  }
  st.state[s] = ST_TRACKED;
  L.tstate[s] = ST_TRACKED;
  st.act[s] = 1;
  st.frame[s] = fid;
  st.score[s] = L.dscore[j];
  st.cls[s] = L.dcls[j];
  st.idx[s] = j;
  L.dused[j] = 1;
}

// weight of (row i, real column c): cost - thresh in fp64, +inf when the pair may not be matched
__device__ __forceinline__ double edge_weight(const Lds& L, int i, int c, int mode, double thresh) {
  const int s = L.rowlist[i], j = L.collist[c];
  float b[4];
  det_xyxy(L.dtlwh + j * 4, b);
  float cost = iou_dist(L.tbox + s * 4, b);
  if (mode == COST_FUSED) {
    const float sim = 1.0f - cost;
    const float fs = sim * L.dscore[j];
    cost = 1.0f - fs;
  }
  const double c64 = (double)cost;
  return (finite_f(cost) && c64 <= thresh) ? c64 - thresh : INFINITY;
}

// Exact rectangular assignment: every row i of L.rowlist[0..nrows) takes a real column c < ncols (weight
// edge_weight) or its own dummy column ncols + i (weight 0), minimising the sum.  Shortest augmenting paths with
// dual variables; the column scan of each Dijkstra step runs over the lanes.  L.col4row[i] < ncols: matched.
__device__ void assign(const Lds& L, Shared& sh, int nrows, int ncols, int mode, double thresh) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int C = ncols + nrows;
  for (int r = t; r < nrows; r += TK_THREADS) {
    L.u[r] = 0.0;
    L.col4row[r] = -1;
  }
  for (int c = t; c < C; c += TK_THREADS) {
    L.v[c] = 0.0;
    L.row4col[c] = -1;
  }
  __syncthreads();
  if (ncols == 0) {  // linear_assignment on an empty matrix: nothing matched
    for (int r = t; r < nrows; r += TK_THREADS) L.col4row[r] = ncols + r;
    __syncthreads();
    return;
  }
  for (int cur = 0; cur < nrows; ++cur) {
    for (int c = t; c < C; c += TK_THREADS) {
      L.spc[c] = INFINITY;
      L.SC[c] = 0;
    }
    for (int r = t; r < nrows; r += TK_THREADS) L.SR[r] = 0;
    __syncthreads();
    double minval = 0.0;
    int i = cur, sink = -1;
    for (int it = 0; it < C && sink < 0; ++it) {
      const double ui = L.u[i];
      double bv = INFINITY;
      int bi = 0x7fffffff, bfree = 0;
      // the real columns over the lanes, the row's own dummy column on lane 0 of the last slot
      for (int c = t; c <= ncols; c += TK_THREADS) {
        const int col = c < ncols ? c : ncols + i;
        if (L.SC[col]) continue;
        const double w = c < ncols ? edge_weight(L, i, c, mode, thresh) : 0.0;
        if (w < INFINITY) {
          const double r = minval + w - ui - L.v[col];
          if (r < L.spc[col]) {
            L.spc[col] = r;
            L.path[col] = i;
          }
        }
      }
      __syncthreads();
      // minimum of spc over the unscanned columns (prefer a free column, then the lower index)
      for (int c = t; c < C; c += TK_THREADS) {
        if (L.SC[c]) continue;
        const double r = L.spc[c];
        const int fr = L.row4col[c] < 0;
        if (r < bv || (r == bv && r < INFINITY && (fr > bfree || (fr == bfree && c < bi)))) {
          bv = r;
          bi = c;
          bfree = fr;
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o), of = __shfl_xor(bfree, o);
        if (ov < bv || (ov == bv && ov < INFINITY && (of > bfree || (of == bfree && oi < bi)))) {
          bv = ov;
          bi = oi;
          bfree = of;
        }
      }
      if (lane == 0) {
        sh.red_val[wave] = bv;
        sh.red_idx[wave] = bi;
        sh.red_free[wave] = bfree;
      }
      __syncthreads();
      bv = sh.red_val[0];
      bi = sh.red_idx[0];
      bfree = sh.red_free[0];
      for (int w = 1; w < TK_WAVES; ++w) {
        const double ov = sh.red_val[w];
        const int oi = sh.red_idx[w], of = sh.red_free[w];
        if (ov < bv || (ov == bv && ov < INFINITY && (of > bfree || (of == bfree && oi < bi)))) {
          bv = ov;
          bi = oi;
          bfree = of;
        }
      }
      if (!(bv < INFINITY)) break;  // cannot happen: the row's dummy column is always reachable
      minval = bv;
      const int nexti = L.row4col[bi];
      __syncthreads();  // every lane has read the reduction and row4col before they change
      if (t == 0) {
        L.SR[i] = 1;
        L.SC[bi] = 1;
      }
      if (nexti < 0) sink = bi;
      else i = nexti;
      __syncthreads();
    }
    if (sink < 0) {  // unreachable guard: leave the row on its dummy
      if (t == 0) L.col4row[cur] = ncols + cur;
      __syncthreads();
      continue;
    }
    // dual update (scipy's rectangular LSAP form), then augment along the path
    for (int r = t; r < nrows; r += TK_THREADS) {
      if (r == cur) L.u[r] += minval;
      else if (L.SR[r]) L.u[r] += minval - L.spc[L.col4row[r]];
    }
    for (int c = t; c < C; c += TK_THREADS)
      if (L.SC[c]) L.v[c] -= minval - L.spc[c];
    __syncthreads();
    if (t == 0) {
      int j = sink;
      for (int it = 0; it <= nrows; ++it) {
        const int r = L.path[j];
        L.row4col[j] = r;
        const int pj = L.col4row[r];
        L.col4row[r] = j;
        j = pj;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
}

// slots s < hwm with pred(s), ordered by their sequence key, into list[base + rank]; returns nothing (counts via cnt)
template <typename Pred>
__device__ inline void ordered_list(const Lds& L, int hwm, int* list, int base, int* cnt, Pred pred) {
  for (int s = threadIdx.x; s < hwm; s += TK_THREADS) {
    if (!pred(s)) continue;
    const long long q = L.tseq[s];
    int rank = 0;
    for (int o = 0; o < hwm; ++o) rank += (pred(o) && L.tseq[o] < q) ? 1 : 0;
    list[base + rank] = s;
    atomicAdd(cnt, 1);
  }
}

// one frame (image `img`) through one tracker
__device__ void track_frame(const TrkParams& p, int img, const StateView& st, const Lds& L, Shared& sh) {
  const int t = threadIdx.x;
  const int D = p.max_det, T = p.T;
  float* out = p.out + (int64_t)img * D * 7;
  int32_t* oidx = p.out_idx ? p.out_idx + (int64_t)img * D : nullptr;
  // ---- header, reset, output rows cleared
  if (t == 0) {
    sh.seqctr = *st.seqctr;
    sh.frame_id = st.head[0];
    sh.next_id = st.head[1];
    sh.overflow = st.head[2];
    sh.hwm = min(max(st.head[3], 0), T);
    int nd = p.det_count[(int64_t)img * p.count_stride];
    sh.nd = min(max(nd, 0), D);
  }
  __syncthreads();
  if (p.reset_each) {
    for (int s = t; s < sh.hwm; s += TK_THREADS) st.state[s] = ST_FREE;
    __syncthreads();
    if (t == 0) {
      sh.seqctr = 0;
      sh.frame_id = sh.next_id = sh.hwm = 0;  // the overflow counter is cumulative
    }
    __syncthreads();
  }
  for (int e = t; e < D * 7; e += TK_THREADS) out[e] = 0.0f;
  if (oidx)
    for (int e = t; e < D; e += TK_THREADS) oidx[e] = -1;
  const int nd = sh.nd;
  if (nd == 0) {  // the reference does not call update(): the frame counter stays
    if (t == 0) {
      p.out_count[img] = 0;
      p.tracked[img] = 0;
      if (p.reset_each) {
        *st.seqctr = 0;
        st.head[0] = st.head[1] = st.head[3] = 0;
      }
    }
    __syncthreads();
    return;
  }
  if (t == 0) sh.frame_id += 1;
  // ---- detections: score split (fp32), xywh -> fp32 _tlwh
  const float* det = p.det + (int64_t)img * p.det_stride;
  for (int j = t; j < nd; j += TK_THREADS) {
    const float x1 = det[j * 6 + 0], y1 = det[j * 6 + 1], x2 = det[j * 6 + 2], y2 = det[j * 6 + 3];
    const float sc = det[j * 6 + 4], cl = det[j * 6 + 5];
    const float cx = (x1 + x2) / 2.0f, cy = (y1 + y2) / 2.0f, w = x2 - x1, h = y2 - y1;
    const float l = (float)((double)cx - (double)w / 2), tp = (float)((double)cy - (double)h / 2);
    L.dtlwh[j * 4 + 0] = l;
    L.dtlwh[j * 4 + 1] = tp;
    L.dtlwh[j * 4 + 2] = w;
    L.dtlwh[j * 4 + 3] = h;
    L.dscore[j] = sc;
    L.dcls[j] = cl;
    const float a = w / h;
    const bool ok = finite_f(l) && finite_f(tp) && finite_f(w) && finite_f(h) && finite_f(a) && finite_f(sc) &&
                    finite_f(cl) && finite_f(w + l) && finite_f(h + tp);
    int kind = 0;
    if (ok) {
      if (sc >= p.high) kind = 1;
      else if (sc > p.low && sc < p.high) kind = 2;
    }
    L.dkind[j] = kind;
    L.dused[j] = 0;
  }
  if (t == 0) sh.npt = sh.npool = sh.nuncf = 0;
  __syncthreads();
  const int hwm = sh.hwm, fid = sh.frame_id;
  for (int s = t; s < hwm; s += TK_THREADS) {
    L.tstate[s] = st.state[s];
    L.tact[s] = st.act[s];
    L.tseq[s] = st.seq[s];
    L.tflag[s] = FL_NONE;
  }
  __syncthreads();
  // ---- strack_pool = activated tracked + lost (list order), unconfirmed = tracked but not activated
  ordered_list(L, hwm, L.pool, 0, &sh.npt, [&](int s) { return L.tstate[s] == ST_TRACKED && L.tact[s] != 0; });
  __syncthreads();
  const int npt = sh.npt;
  ordered_list(L, hwm, L.pool, npt, &sh.npool, [&](int s) { return L.tstate[s] >= ST_LOST; });
  ordered_list(L, hwm, L.uncf, 0, &sh.nuncf, [&](int s) { return L.tstate[s] == ST_TRACKED && L.tact[s] == 0; });
  __syncthreads();
  const int npool = npt + sh.npool, nuncf = sh.nuncf;
  // ---- multi_predict over the pool; boxes of pool and unconfirmed tracks
  for (int r = t; r < npool + nuncf; r += TK_THREADS) {
    const int s = r < npool ? L.pool[r] : L.uncf[r - npool];
    if (r < npool) kf_predict(st, s, L.tstate[s] != ST_TRACKED);
    slot_box(st, L, s);
  }
  // ---- first association: pool x high detections, fused score, match_thresh
  for (int r = t; r < npool; r += TK_THREADS) L.rowlist[r] = L.pool[r];
  if (t == 0) sh.ncols = 0;
  __syncthreads();
  for (int j = t; j < nd; j += TK_THREADS) {
    if (L.dkind[j] != 1) continue;
    int rank = 0;
    for (int o = 0; o < j; ++o) rank += L.dkind[o] == 1;
    L.collist[rank] = j;
    atomicAdd(&sh.ncols, 1);
  }
  __syncthreads();
  int ncols = sh.ncols;
  assign(L, sh, npool, ncols, p.fuse ? COST_FUSED : COST_IOU, p.match);
  for (int r = t; r < npool; r += TK_THREADS) {
    const int c = L.col4row[r];
    L.SR[r] = (c >= 0 && c < ncols) ? 1 : 0;  // matched in the first association (SR is free between assignments)
    if (L.SR[r]) apply_match(st, L, L.pool[r], L.collist[c], fid);
  }
  if (t == 0) sh.nrows = sh.ncols = 0;
  __syncthreads();
  // ---- second association: the unmatched pool tracks that were Tracked x low detections, IoU, 0.5
  for (int r = t; r < npool; r += TK_THREADS) {
    if (L.SR[r] || L.tstate[L.pool[r]] != ST_TRACKED) continue;
    int rank = 0;
    for (int o = 0; o < r; ++o) rank += (!L.SR[o] && L.tstate[L.pool[o]] == ST_TRACKED) ? 1 : 0;
    L.rowlist[rank] = L.pool[r];
    atomicAdd(&sh.nrows, 1);
  }
  for (int j = t; j < nd; j += TK_THREADS) {
    if (L.dkind[j] != 2) continue;
    int rank = 0;
    for (int o = 0; o < j; ++o) rank += L.dkind[o] == 2;
    L.collist[rank] = j;
    atomicAdd(&sh.ncols, 1);
  }
  __syncthreads();
  int nrows = sh.nrows;
  ncols = sh.ncols;
  assign(L, sh, nrows, ncols, COST_IOU, 0.5);
  for (int r = t; r < nrows; r += TK_THREADS) {
    const int c = L.col4row[r], s = L.rowlist[r];
    if (c >= 0 && c < ncols) {
      apply_match(st, L, s, L.collist[c], fid);
    } else if (st.rmem[s]) {  // its id is in removed_stracks: sub_stracks drops it from the lost list at once
      st.state[s] = ST_FREE;
      L.tstate[s] = ST_FREE;
    } else {
      st.state[s] = ST_LOST;
      L.tstate[s] = ST_LOST;
      L.tflag[s] = FL_NEWLOST;
    }
  }
  if (t == 0) sh.ncols = 0;
  __syncthreads();
  // ---- unconfirmed x left-over high detections, fused score, 0.7
  for (int r = t; r < nuncf; r += TK_THREADS) L.rowlist[r] = L.uncf[r];
  for (int j = t; j < nd; j += TK_THREADS) {
    if (L.dkind[j] != 1 || L.dused[j]) continue;
    int rank = 0;
    for (int o = 0; o < j; ++o) rank += (L.dkind[o] == 1 && !L.dused[o]) ? 1 : 0;
    L.collist[rank] = j;
    atomicAdd(&sh.ncols, 1);
  }
  __syncthreads();
  ncols = sh.ncols;
  assign(L, sh, nuncf, ncols, p.fuse ? COST_FUSED : COST_IOU, 0.7);
  for (int r = t; r < nuncf; r += TK_THREADS) {
    const int c = L.col4row[r], s = L.uncf[r];
    if (c >= 0 && c < ncols) {
      apply_match(st, L, s, L.collist[c], fid);
    } else {  // mark_removed: in no list any more
      st.state[s] = ST_FREE;
      L.tstate[s] = ST_FREE;
    }
  }
  __syncthreads();
  // ---- new tracks from the left-over high detections (ascending), lowest free slot each; then the sequence keys of
  // the re-found and the newly lost tracks in pool order (short serial bookkeeping on one lane)
  if (t == 0) {
    int cursor = 0, nnew = 0;
    for (int j = 0; j < nd; ++j) {
      if (L.dkind[j] != 1 || L.dused[j]) continue;
      if (L.dscore[j] < p.newt) continue;
      while (cursor < T && cursor < sh.hwm && L.tstate[cursor] != ST_FREE) ++cursor;
      if (cursor >= T) {
        sh.overflow += 1;
        continue;
      }
      const int s = cursor++;
      if (s >= sh.hwm) sh.hwm = s + 1;
      L.tstate[s] = ST_TRACKED;
      L.tflag[s] = FL_NONE;
      L.path[nnew] = s;
      L.row4col[nnew] = j;
      st.id[s] = ++sh.next_id;
      st.seq[s] = sh.seqctr++;
      ++nnew;
    }
    sh.nnew = nnew;
    for (int r = 0; r < npool; ++r) {
      const int s = L.pool[r];
      if (L.tflag[s] == FL_REFIND) st.seq[s] = sh.seqctr++;
    }
    for (int r = 0; r < npool; ++r) {
      const int s = L.pool[r];
      if (L.tflag[s] == FL_NEWLOST) st.seq[s] = sh.seqctr++;
    }
  }
  __syncthreads();
  for (int k = t; k < sh.nnew; k += TK_THREADS) {
    const int s = L.path[k], j = L.row4col[k];
    kf_initiate(st, s, L.dtlwh + j * 4);
    st.state[s] = ST_TRACKED;
    st.act[s] = fid == 1 ? 1 : 0;
    st.frame[s] = fid;
    st.start[s] = fid;
    st.tlen[s] = 0;
    st.idx[s] = j;
    st.rmem[s] = 0;
    st.score[s] = L.dscore[j];
    st.cls[s] = L.dcls[j];
  }
  if (t == 0) sh.na = sh.nb = sh.nout = 0;
  __syncthreads();
  const int hwm2 = sh.hwm;
  // ---- lost list: zombies of earlier frames leave (sub_stracks with removed_stracks), lost tracks past
  // max_time_lost are marked removed (they stay listed for one more frame, as in the reference)
  for (int s = t; s < hwm2; s += TK_THREADS) {
    const int state = L.tstate[s];
    if (state == ST_REMOVED) {
      st.state[s] = ST_FREE;
      L.tstate[s] = ST_FREE;
    } else if (state == ST_LOST && L.tflag[s] != FL_NEWLOST && fid - st.frame[s] > p.max_time_lost) {
      st.state[s] = ST_REMOVED;
      L.tstate[s] = ST_REMOVED;
      st.rmem[s] = 1;
    }
  }
  __syncthreads();
  // ---- remove_duplicate_stracks(tracked, lost): IoU distance < 0.15, the younger goes (on equal age the tracked)
  for (int s = t; s < hwm2; s += TK_THREADS) {
    const int state = L.tstate[s];
    L.SR[s] = 0;
    if (state == ST_FREE) continue;
    slot_box(st, L, s);
    if (state == ST_TRACKED) L.rowlist[atomicAdd(&sh.na, 1)] = s;
    else L.pool[atomicAdd(&sh.nb, 1)] = s;
  }
  __syncthreads();
  {
    const int na = sh.na, nb = sh.nb;
    for (int64_t e = t; e < (int64_t)na * nb; e += TK_THREADS) {
      const int a = L.rowlist[e / nb], b = L.pool[e % nb];
      const float dist = iou_dist(L.tbox + a * 4, L.tbox + b * 4);
      if (dist < 0.15f) {
        const int ta = st.frame[a] - st.start[a], tb = st.frame[b] - st.start[b];
        L.SR[ta > tb ? b : a] = 1;
      }
    }
  }
  __syncthreads();
  for (int s = t; s < hwm2; s += TK_THREADS) {
    if (L.SR[s]) {
      st.state[s] = ST_FREE;
      L.tstate[s] = ST_FREE;
    }
    L.tact[s] = st.act[s];
    L.tseq[s] = st.seq[s];
  }
  __syncthreads();
  // ---- output: the activated tracked tracks in list order, x1 y1 x2 y2 id conf cls, clipped to the image
  const float ih = p.hw[img * 2 + 0], iw = p.hw[img * 2 + 1];
  for (int s = t; s < hwm2; s += TK_THREADS) {
    if (L.tstate[s] != ST_TRACKED || !L.tact[s]) continue;
    const long long q = L.tseq[s];
    int rank = 0;
    for (int o = 0; o < hwm2; ++o) rank += (L.tstate[o] == ST_TRACKED && L.tact[o] && L.tseq[o] < q) ? 1 : 0;
    atomicAdd(&sh.nout, 1);
    if (rank >= D) continue;
    double b[4];
    mean_xyxy(st.mean + (int64_t)s * 8, b);
    float* row = out + rank * 7;
    row[0] = fminf(fmaxf((float)b[0], 0.0f), iw);
    row[1] = fminf(fmaxf((float)b[1], 0.0f), ih);
    row[2] = fminf(fmaxf((float)b[2], 0.0f), iw);
    row[3] = fminf(fmaxf((float)b[3], 0.0f), ih);
    row[4] = (float)st.id[s];
    row[5] = st.score[s];
    row[6] = st.cls[s];
    if (oidx) oidx[rank] = st.idx[s];
  }
  __syncthreads();
  if (t == 0) {
    const int nout = min(sh.nout, D);
    p.out_count[img] = nout;
    p.tracked[img] = nout > 0 ? 1 : 0;
    *st.seqctr = sh.seqctr;
    st.head[0] = sh.frame_id;
    st.head[1] = sh.next_id;
    st.head[2] = sh.overflow;
    st.head[3] = sh.hwm;
  }
  __syncthreads();
}

__global__ __launch_bounds__(TK_THREADS) void bytetrack_kernel(TrkParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tk_lds[];
  __shared__ Shared sh;
  const Lds L = carve(tk_lds, p.T, p.max_det);
  const int k = blockIdx.x;
  const StateView st = state_view(p.state + (int64_t)k * p.state_bytes, p.T);
  if (p.trackers == 1) {
    for (int img = 0; img < p.n; ++img) track_frame(p, img, st, L, sh);  // the batch's rows are consecutive frames
  } else {
    track_frame(p, k, st, L, sh);
  }
}

}  // namespace
}  // namespace ydbl

using namespace ydbl;

extern "C" int64_t ydbl_bytetrack_state_bytes(int32_t max_tracks, int32_t max_det) {
  if (max_tracks < 1 || max_det < 1) return -1;
  return tk_state_bytes(max_tracks);  // per tracker; nothing in it is sized by max_det
}

extern "C" int ydbl_bytetrack_update(const ydbl_track_desc* d, void* stream) {
  if (!d) return fail(YDBL_EINVAL, "bytetrack_update: null descriptor");
  if (!d->det || !d->det_count || !d->hw || !d->out || !d->out_count || !d->tracked || !d->state)
    return fail(YDBL_EINVAL, "bytetrack_update: null pointer");
  if (d->n < 1 || d->max_det < 1) return fail(YDBL_EINVAL, "bytetrack_update: n and max_det must be >= 1");
  if (d->max_tracks < 1) return fail(YDBL_EINVAL, "bytetrack_update: max_tracks must be >= 1");
  if (d->trackers != 1 && d->trackers != d->n)
    return fail(YDBL_EINVAL, "bytetrack_update: trackers must be 1 (the rows are consecutive frames) or n (one "
                             "tracker per row), got " + std::to_string(d->trackers));
  if (d->trackers > 65535) return fail(YDBL_EINVAL, "bytetrack_update: more than 65535 trackers");
  const int64_t dstride = d->det_stride ? d->det_stride : (int64_t)d->max_det * 6;
  const int64_t cstride = d->count_stride ? d->count_stride : 1;
  if (dstride < (int64_t)d->max_det * 6 || cstride < 1)
    return fail(YDBL_EINVAL, "bytetrack_update: det_stride < max_det * 6 or count_stride < 1");
  if (!(d->track_high_thresh >= 0 && d->track_high_thresh <= 1) || !(d->track_low_thresh >= 0 && d->track_low_thresh <= 1) ||
      !(d->new_track_thresh >= 0 && d->new_track_thresh <= 1) || !(d->match_thresh >= 0 && d->match_thresh <= 1))
    return fail(YDBL_EINVAL, "bytetrack_update: thresholds must lie in [0, 1]");
  if (d->max_time_lost < 0 || d->track_buffer < 0)
    return fail(YDBL_EINVAL, "bytetrack_update: track_buffer and max_time_lost must be >= 0");
  const int64_t sbytes = ydbl_bytetrack_state_bytes(d->max_tracks, d->max_det);
  if (d->state_bytes < sbytes * d->trackers)
    return fail(YDBL_EINVAL, "bytetrack_update: state buffer smaller than trackers * ydbl_bytetrack_state_bytes = " +
                                 std::to_string(sbytes * d->trackers) + " bytes");
  if (reinterpret_cast<uintptr_t>(d->state) % 16) return fail(YDBL_EINVAL, "bytetrack_update: state not 16-byte aligned");
  const int64_t lds = tk_lds_bytes(d->max_tracks, d->max_det);
  if (lds > 160 * 1024)
    return fail(YDBL_ECAPACITY, "bytetrack_update: max_tracks + max_det need " + std::to_string(lds) +
                                    " bytes of LDS, more than the 160 KiB of a workgroup");
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(bytetrack_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(YDBL_ELAUNCH, std::string("bytetrack_update: ") + hipGetErrorString(e));
  }
  TrkParams p;
  p.det = d->det;
  p.det_count = d->det_count;
  p.hw = d->hw;
  p.n = d->n;
  p.max_det = d->max_det;
  p.det_stride = dstride;
  p.count_stride = cstride;
  p.high = (float)d->track_high_thresh;
  p.low = (float)d->track_low_thresh;
  p.newt = (float)d->new_track_thresh;
  p.match = d->match_thresh;
  p.fuse = d->fuse_score;
  p.max_time_lost = d->max_time_lost;
  p.T = d->max_tracks;
  p.trackers = d->trackers;
  p.reset_each = d->reset_each;
  p.out = d->out;
  p.out_count = d->out_count;
  p.tracked = d->tracked;
  p.out_idx = d->out_idx;
  p.state = reinterpret_cast<unsigned char*>(d->state);
  p.state_bytes = sbytes;
  bytetrack_kernel<<<dim3(d->trackers), TK_THREADS, (size_t)lds, as_stream(stream)>>>(p);
  return check_launch("ydbl_bytetrack_update");
}
