// The per-anchor arithmetic of the Detect decode (U/nn/modules/head.py:143-181, DFL block.py:79-83, dist2bbox
// utils/tal.py:333-357, the NMS candidate filter utils/ops.py:234-276), shared by the decode kernels (detect.hip) and
// the class-conv tail of the DSConv kernels (conv_common.hpp), which emits the candidates itself.
//
// detect.hip is compiled without fp contraction, the convolution sources with it: every function here that
// multiplies and adds switches it off in its own body, so both callers produce the same bits.
#pragma once
#include "common.hpp"

namespace ydbl {

// The candidate lists of ydbl_decode_desc (per image `cap` entries and one counter) and the filter that fills them.
struct CandSink {
  float* cbox; float* cscore; int* ccls; int* cidx; int* ccount;
  int cap;
  float conf;
  int multi;
  const int* classes; int ncls;
};

// Slot of this lane's candidate in image b's list: one atomic per wave (the first active lane adds the
// wave's candidate count, the others take their rank among the active lanes).  Candidates cluster on
// objects, so a wave often holds tens of them; per-lane atomics on the one counter serialize in L2.
__device__ __forceinline__ int wave_slot(int* counter, bool want) {
  const uint64_t m = __ballot(want);
  if (!want) return -1;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(m));
  base = __shfl(base, leader);
  return base + __popcll(m & ((1ull << lane) - 1));
}

__device__ __forceinline__ bool class_ok(int j, const int* classes, int ncls) {
  if (!classes) return true;
  for (int q = 0; q < ncls; ++q)
    if (classes[q] == j) return true;
  return false;
}

// DFL of one box side: softmax over its 16 bins (bp: the side's 16 logits), expectation with weights 0..15
template <typename T>
__device__ __forceinline__ float dfl_side(const T* bp) {
#pragma clang fp contract(off)
  float v[16];
  load_f<8>(bp, v);
  load_f<8>(bp + 8, v + 8);
  float m = v[0];
#pragma unroll
  for (int k = 1; k < 16; ++k) m = fmaxf(m, v[k]);
  float e[16], sum = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    e[k] = expf(v[k] - m);
    sum += e[k];
  }
  // softmax weights as e * (1 / sum): one division per side instead of 16 (<= 1 ulp per weight, far
  // inside the decode tolerance; the reference's DFL conv sums the 16 products in its own order anyway)
  const float inv = 1.0f / sum;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) acc += float(k) * (e[k] * inv);
  return acc;
}

struct Xywh {
  float cx, cy, w, h;
};

// anchor point (gx + 0.5, gy + 0.5), dist2bbox (xywh) and the level's stride
__device__ __forceinline__ Xywh dist2xywh(int gx, int gy, const float (&dist)[4], float st) {
#pragma clang fp contract(off)
  const float ax = float(gx) + 0.5f, ay = float(gy) + 0.5f;
  const float x1 = ax - dist[0], y1 = ay - dist[1], x2 = ax + dist[2], y2 = ay + dist[3];
  Xywh o;
  o.cx = ((x1 + x2) / 2.0f) * st;
  o.cy = ((y1 + y2) / 2.0f) * st;
  o.w = (x2 - x1) * st;
  o.h = (y2 - y1) * st;
  return o;
}

// dist2bbox(xywh=False) * stride, the end2end head's decode (head.py:196-198, utils/tal.py:333-357): the corners
// straight from the distances, (anchor -+ dist) * stride, never through xywh
__device__ __forceinline__ f32x4 dist2xyxy(int gx, int gy, const float (&dist)[4], float st) {
#pragma clang fp contract(off)
  const float ax = float(gx) + 0.5f, ay = float(gy) + 0.5f;
  return f32x4{(ax - dist[0]) * st, (ay - dist[1]) * st, (ax + dist[2]) * st, (ay + dist[3]) * st};
}

// xywh2xyxy (U/utils/ops.py:416-433)
__device__ __forceinline__ f32x4 xywh2xyxy(const Xywh& v) {
#pragma clang fp contract(off)
  const float hw = v.w / 2.0f, hh = v.h / 2.0f;
  return f32x4{v.cx - hw, v.cy - hh, v.cx + hw, v.cy + hh};
}

__device__ __forceinline__ float cls_score(float logit) {
#pragma clang fp contract(off)
  return 1.0f / (1.0f + expf(-logit));
}

// The quad's first maximum (torch.max: larger score, or the same score at a smaller class index); the quad's
// lanes are QS lanes apart.
template <int QS>
__device__ __forceinline__ void quad_first_max(float& best, int& bj) {
#pragma unroll
  for (int k = 1; k < 4; k <<= 1) {
    const float ob = __shfl_xor(best, k * QS);
    const int oj = __shfl_xor(bj, k * QS);
    if (ob > best || (ob == best && oj < bj)) {
      best = ob;
      bj = oj;
    }
  }
}

__device__ __forceinline__ void cand_write(const CandSink& k, int b, int slot, const f32x4& box, float sc, int cls,
                                           int idx) {
  if (slot >= 0 && slot < k.cap) {
    const int64_t o = (int64_t)b * k.cap + slot;
    *reinterpret_cast<f32x4*>(k.cbox + o * 4) = box;
    k.cscore[o] = sc; k.ccls[o] = cls; k.cidx[o] = idx;
  }
}

// cand_write without the box: the deferred sink (the level's box launch fills cand_box afterwards, bneck.hip)
__device__ __forceinline__ void cand_write_nobox(const CandSink& k, int b, int slot, float sc, int cls, int idx) {
  if (slot >= 0 && slot < k.cap) {
    const int64_t o = (int64_t)b * k.cap + slot;
    k.cscore[o] = sc; k.ccls[o] = cls; k.cidx[o] = idx;
  }
}

// One anchor's candidates, classes first: the four lanes of a quad call it together (lane s = side s and the
// classes s, s + 4, ...; the quad's lanes are QS apart in the wave).  The box -- 64 logits read, 64 exponentials --
// is decoded only in quads that hold a candidate (a percent or two of the anchors at predict thresholds); the
// scores, the filter and the box arithmetic are the box-first decode's, value for value.
//   ok      false (for all four lanes): the quad is no anchor and offers nothing
//   logit   j -> class j's logit as stored (the activation dtype's value)
//   bp      the anchor's 64 box logits (16-byte aligned); read only where the quad holds a candidate
//   pos     the anchor's candidate index (pos * nc + class when multi-label)
// DEFER (the sparse box path): same filter, same scores, same slots, but no box is read or written; a quad that holds
// a candidate stores 1 into *tile, the mask byte of the anchor's 8 x 16 tile (racing quads store the same value).
// XYXY: the end2end head's boxes (dist2xyxy).
template <typename T, int QS, bool DEFER = false, bool XYXY = false, typename F>
__device__ __forceinline__ void quad_candidates(const CandSink& k, int b, int s, bool ok, int nc, F&& logit,
                                                const T* bp, int gx, int gy, float st, int pos,
                                                unsigned char* tile = nullptr) {
  float best = -1.f;
  int bj = 0;
  int any = 0;
  for (int j = s; j < nc; j += 4) {
    const float sc = cls_score(logit(j));
    if (k.multi) {
      any |= sc > k.conf && class_ok(j, k.classes, k.ncls);
    } else if (sc > best) {  // torch.max: first index of the maximum (within this lane's classes)
      best = sc;
      bj = j;
    }
  }
  bool want;  // the quad holds a candidate
  if (k.multi) {
    any |= __shfl_xor(any, QS);
    any |= __shfl_xor(any, 2 * QS);
    want = ok && any;
  } else {
    quad_first_max<QS>(best, bj);
    want = ok && best > k.conf && class_ok(bj, k.classes, k.ncls);
  }
  if constexpr (DEFER) {
    if (want) {  // whole quads
      if (s == 0) *tile = 1;
      if (k.multi) {
        for (int j = s; j < nc; j += 4) {
          const float sc = cls_score(logit(j));
          const int slot = wave_slot(k.ccount + b, sc > k.conf && class_ok(j, k.classes, k.ncls));
          cand_write_nobox(k, b, slot, sc, j, pos * nc + j);
        }
      }
    }
    if (k.multi) return;
    const int slot = wave_slot(k.ccount + b, s == 0 && want);
    cand_write_nobox(k, b, slot, best, bj, pos);
    return;
  }
  f32x4 box = f32x4{0.f, 0.f, 0.f, 0.f};
  if (want) {  // whole quads
    const float mine = dfl_side(bp + s * 16);
    const int q0 = (threadIdx.x & 63) - s * QS;  // the quad's first lane
    float dist[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dist[i] = __shfl(mine, q0 + i * QS);
    if constexpr (XYXY) box = dist2xyxy(gx, gy, dist, st);
    else box = xywh2xyxy(dist2xywh(gx, gy, dist, st));
    if (k.multi) {
      for (int j = s; j < nc; j += 4) {
        const float sc = cls_score(logit(j));
        const int slot = wave_slot(k.ccount + b, sc > k.conf && class_ok(j, k.classes, k.ncls));
        cand_write(k, b, slot, box, sc, j, pos * nc + j);
      }
    }
  }
  if (k.multi) return;
  const int slot = wave_slot(k.ccount + b, s == 0 && want);
  cand_write(k, b, slot, box, best, bj, pos);
}

}  // namespace ydbl
