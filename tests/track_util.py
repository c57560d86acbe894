"""ByteTrack restated in numpy / scipy for the tracking tests, plus the scenes they share.

Written from the reference's trackers (U/trackers/track.py:18-87, byte_tracker.py:51-228 and :293-405,
utils/kalman_filter.py:52-236, utils/matching.py:20-61, 64-101, 134-157), as oracle/ops.py restates its NMS:
  - the tracker keeps the reference's three lists as Python lists of track records and walks them in its order;
  - detections: fp32 xyxy -> fp32 xywh -> (fp64) ltwh rounded to the fp32 ``_tlwh``; xyah in fp32;
  - Kalman state fp64, with the fp32 roundings of ``initiate`` (mean, and the std products under NEP 50);
    predict / project / update in fp64 (Cholesky through scipy, as the reference);
  - IoU distance and fused score in fp32, numpy's operation order; score comparisons in fp32;
  - the assignment: ``lap.lapjv(cost, extend_cost=True, cost_limit=L)`` minimises sum_matched (c - L); here it is
    scipy.optimize.linear_sum_assignment on the extended square matrix [[C, L/2], [L/2, 0]].
Rules of ours that the device kernel shares (include/ydbl.h): a detection with a non-finite box, score or class, or
of zero height, takes no part; ``max_tracks`` live tracks at most (then no new track, ``overflow`` += 1, no id
spent); the removed list is a set of ids, never cut at 1000.

The tracker also records what the tests need to know about their *inputs*: which branches fired, the uniqueness
margin of every assignment (best objective with a chosen pair forbidden, minus the optimum; minimum over the chosen
pairs), the smallest distance of any threshold comparison from its threshold, and every cost matrix.
"""

from __future__ import annotations

from collections import Counter

import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.optimize import linear_sum_assignment

CFG = {"tracker_type": "bytetrack", "track_high_thresh": 0.25, "track_low_thresh": 0.1, "new_track_thresh": 0.25,
       "track_buffer": 30, "match_thresh": 0.8, "fuse_score": True}
TRACKED, LOST, REMOVED = 1, 2, 3
F32 = np.float32
W_POS, W_VEL = 1.0 / 20, 1.0 / 160


# ------------------------------------------------------------------------------------------ Kalman filter (xyah)
def kf_initiate(z32):
    mean = np.concatenate([z32.astype(np.float64), np.zeros(4)])  # fp32 values
    sp = float(F32(2 * W_POS) * z32[3])    # python float * np.float32 is an fp32 product (NEP 50)
    sv = float(F32(10 * W_VEL) * z32[3])
    std = np.array([sp, sp, 1e-2, sp, sv, sv, 1e-5, sv], dtype=np.float64)
    return mean, np.diag(np.square(std))


_F = np.eye(8)
_F[:4, 4:] = np.eye(4)


def kf_predict(mean, cov):
    h = mean[3]
    std = np.array([W_POS * h, W_POS * h, 1e-2, W_POS * h, W_VEL * h, W_VEL * h, 1e-5, W_VEL * h])
    return mean @ _F.T, _F @ cov @ _F.T + np.diag(np.square(std))


def kf_update(mean, cov, z32):
    h = mean[3]
    std = np.array([W_POS * h, W_POS * h, 1e-1, W_POS * h])
    pm, pc = mean[:4].copy(), cov[:4, :4] + np.diag(np.square(std))
    gain = cho_solve(cho_factor(pc, lower=True, check_finite=False), cov[:, :4].T, check_finite=False).T
    return mean + (z32.astype(np.float64) - pm) @ gain.T, cov - gain @ (pc @ gain.T)


# ------------------------------------------------------------------------------------------ boxes and costs
def det_tlwh(xyxy32):
    """Boxes.xywh (fp32) -> xywh2ltwh in fp64 -> the fp32 _tlwh of STrack.__init__."""
    x1, y1, x2, y2 = (F32(v) for v in xyxy32)
    with np.errstate(all="ignore"):  # non-finite detections are dropped by the caller
        cx, cy, w, h = (x1 + x2) / F32(2), (y1 + y2) / F32(2), x2 - x1, y2 - y1
        return np.array([np.float64(cx) - np.float64(w) / 2, np.float64(cy) - np.float64(h) / 2, w, h]).astype(F32)


def tlwh_xyah(t32):
    return np.array([t32[0] + t32[2] / F32(2), t32[1] + t32[3] / F32(2), t32[2] / t32[3], t32[3]], dtype=F32)


def mean_xyxy(mean):
    w = mean[2] * mean[3]
    x1, y1 = mean[0] - w / 2, mean[1] - mean[3] / 2
    return np.array([x1, y1, w + x1, mean[3] + y1])


def iou_distance(a, b):
    """1 - bbox_ioa(a, b, iou=True) in fp32; a [n,4], b [m,4] xyxy."""
    a, b = np.asarray(a, dtype=F32).reshape(-1, 4), np.asarray(b, dtype=F32).reshape(-1, 4)
    if not len(a) or not len(b):
        return np.zeros((len(a), len(b)), dtype=F32)
    ax1, ay1, ax2, ay2 = a.T
    bx1, by1, bx2, by2 = b.T
    inter = (np.minimum(ax2[:, None], bx2) - np.maximum(ax1[:, None], bx1)).clip(0) * \
            (np.minimum(ay2[:, None], by2) - np.maximum(ay1[:, None], by1)).clip(0)
    area = (bx2 - bx1) * (by2 - by1)
    area = area + ((ax2 - ax1) * (ay2 - ay1))[:, None] - inter
    return F32(1) - inter / (area + F32(1e-7))


def fuse(cost, scores32):
    if cost.size == 0:
        return cost
    return F32(1) - (F32(1) - cost) * np.asarray(scores32, dtype=F32)[None, :]


# ------------------------------------------------------------------------------------------ the assignment
def _lsa(C, L):
    n, m = C.shape
    ext = np.full((n + m, n + m), L / 2, dtype=np.float64)
    ext[:n, :m] = C
    ext[n:, m:] = 0.0
    r, c = linear_sum_assignment(ext)
    pairs = [(int(i), int(j)) for i, j in zip(r, c) if i < n and j < m]
    return pairs, float(sum(C[i, j] - L for i, j in pairs))


def assignment(C, L):
    """-> (pairs, unmatched rows, unmatched columns, margin).  The optimum of sum_matched (c - L); margin = the
    smallest loss from forbidding one chosen pair (inf without pairs).  Forbidding a pair only touches its connected
    component of the allowed (c <= L) pairs, so the re-solve runs on that component."""
    C = np.asarray(C, dtype=np.float64)
    n, m = C.shape
    if C.size == 0:
        return [], list(range(n)), list(range(m)), np.inf
    pairs, _ = _lsa(C, L)
    # components of the bipartite graph of allowed pairs
    comp_r, comp_c, k = -np.ones(n, int), -np.ones(m, int), 0
    allowed = C <= L
    for i0 in range(n):
        if comp_r[i0] >= 0 or not allowed[i0].any():
            continue
        rows, cols, stack = {i0}, set(), [("r", i0)]
        while stack:
            kind, x = stack.pop()
            nb = np.flatnonzero(allowed[x]) if kind == "r" else np.flatnonzero(allowed[:, x])
            for y in nb:
                tgt = cols if kind == "r" else rows
                if int(y) not in tgt:
                    tgt.add(int(y))
                    stack.append(("c" if kind == "r" else "r", int(y)))
        comp_r[list(rows)] = k
        comp_c[list(cols)] = k
        k += 1
    margin = np.inf
    for i, j in pairs:
        rs, cs = np.flatnonzero(comp_r == comp_r[i]), np.flatnonzero(comp_c == comp_r[i])
        sub = C[np.ix_(rs, cs)].copy()
        _, base = _lsa(sub, L)
        sub[int(np.flatnonzero(rs == i)[0]), int(np.flatnonzero(cs == j)[0])] = 1e9
        _, alt = _lsa(sub, L)
        margin = min(margin, alt - base)
    mr, mc = {i for i, _ in pairs}, {j for _, j in pairs}
    return pairs, [i for i in range(n) if i not in mr], [j for j in range(m) if j not in mc], margin


def greedy_pairs(C, L):
    """Greedy by lowest cost (not what the tracker does): the crossing scene shows it differs from the optimum."""
    C = np.asarray(C, dtype=np.float64)
    order = sorted((C[i, j], i, j) for i in range(C.shape[0]) for j in range(C.shape[1]) if C[i, j] <= L)
    ur, uc, out = set(), set(), []
    for _, i, j in order:
        if i not in ur and j not in uc:
            out.append((i, j))
            ur.add(i)
            uc.add(j)
    return sorted(out)


# ------------------------------------------------------------------------------------------ the tracker
class Track:
    def __init__(self, tlwh32, score, cls, idx):
        self.tlwh32, self.score, self.cls, self.idx = tlwh32, F32(score), F32(cls), int(idx)
        self.mean = self.cov = None
        self.activated, self.state, self.tid = False, 0, 0
        self.frame = self.start = self.tlen = 0

    @property
    def xyxy(self):
        if self.mean is None:
            t = self.tlwh32
            return np.array([t[0], t[1], t[2] + t[0], t[3] + t[1]], dtype=F32)
        return mean_xyxy(self.mean)

    def age(self):
        return self.frame - self.start


class RefTracker:
    def __init__(self, cfg=None, max_tracks=512):
        self.cfg = {**CFG, **(cfg or {})}
        self.max_tracks = max_tracks
        self.max_time_lost = int(30 / 30.0 * self.cfg["track_buffer"])
        self.branches, self.margins, self.costs = Counter(), [], []
        self.near = np.inf  # smallest |value - threshold| over every threshold comparison made
        self.overflow = 0
        self.reset()

    def reset(self):
        self.tracked, self.lost, self.removed_ids = [], [], set()
        self.frame_id = self.next_id = 0

    # -- bookkeeping of the input conditions
    def _cmp(self, values, thr):
        v = np.asarray(values, dtype=np.float64).ravel()
        if v.size:
            self.near = min(self.near, float(np.abs(v - thr).min()))

    def _assign(self, stage, C, L):
        pairs, ur, uc, margin = assignment(C, L)
        self.costs.append((self.frame_id, stage, np.array(C, dtype=np.float64), L, sorted(pairs)))
        if pairs:
            self.margins.append(margin)
        mask = np.ones(np.shape(C), bool)
        for i, j in pairs:
            mask[i, j] = False
        self._cmp(np.asarray(C, dtype=np.float64)[mask], L)
        return pairs, ur, uc

    def _dists(self, tracks, dets):
        d = iou_distance([t.xyxy for t in tracks], [t.xyxy for t in dets])
        return fuse(d, [t.score for t in dets]) if self.cfg["fuse_score"] else d

    def _update_track(self, t, det):
        t.mean, t.cov = kf_update(t.mean, t.cov, tlwh_xyah(det.tlwh32))
        if t.state == TRACKED:
            t.tlen += 1
        else:
            t.tlen = 0
        t.state, t.activated, t.frame = TRACKED, True, self.frame_id
        t.score, t.cls, t.idx = det.score, det.cls, det.idx

    def update(self, det):
        """det [n, 6] fp32 (n >= 1) -> rows [k, 8] fp32: x1, y1, x2, y2, id, score, cls, idx (unclipped)."""
        cfg = self.cfg
        det = np.asarray(det, dtype=F32).reshape(-1, 6)
        self.frame_id += 1
        scores = det[:, 4]
        tl = [det_tlwh(d[:4]) for d in det]
        with np.errstate(all="ignore"):
            ok = np.array([bool(np.isfinite(d).all() and np.isfinite(t).all() and np.isfinite(t[2] / t[3])
                                and np.isfinite(t[2] + t[0]) and np.isfinite(t[3] + t[1])) for d, t in zip(det, tl)])
        self._cmp(scores[ok], cfg["track_high_thresh"])
        self._cmp(scores[ok], cfg["track_low_thresh"])
        high = ok & (scores >= F32(cfg["track_high_thresh"]))
        low = ok & (scores > F32(cfg["track_low_thresh"])) & (scores < F32(cfg["track_high_thresh"]))
        mk = lambda sel: [Track(tl[i], det[i, 4], det[i, 5], i) for i in np.flatnonzero(sel)]  # noqa: E731
        dets, dets2 = mk(high), mk(low)
        activated, refind, lost_now = [], [], []
        unconfirmed = [t for t in self.tracked if not t.activated]
        pool = [t for t in self.tracked if t.activated] + list(self.lost)
        for t in pool:  # multi_predict
            m = t.mean.copy()
            if t.state != TRACKED:
                m[7] = 0
            t.mean, t.cov = kf_predict(m, t.cov)
        # first association
        pairs, u_track, u_det = self._assign("first", self._dists(pool, dets), cfg["match_thresh"])
        for i, j in pairs:
            t = pool[i]
            if t.state == TRACKED:
                self.branches["first_match"] += 1
                activated.append(t)
            else:
                self.branches["refind_removed" if t.state == REMOVED else "refind"] += 1
                refind.append(t)
            self._update_track(t, dets[j])
        # second association
        r_tracked = [pool[i] for i in u_track if pool[i].state == TRACKED]
        d2 = iou_distance([t.xyxy for t in r_tracked], [t.xyxy for t in dets2])
        pairs, u_track2, _ = self._assign("second", d2, 0.5)
        for i, j in pairs:
            self.branches["second_match"] += 1
            self._update_track(r_tracked[i], dets2[j])
            activated.append(r_tracked[i])
        for i in u_track2:
            r_tracked[i].state = LOST
            lost_now.append(r_tracked[i])
            self.branches["lost"] += 1
        # unconfirmed
        dets = [dets[j] for j in u_det]
        pairs, u_unc, u_det = self._assign("unconfirmed", self._dists(unconfirmed, dets), 0.7)
        for i, j in pairs:
            self.branches["confirm"] += 1
            self._update_track(unconfirmed[i], dets[j])
            activated.append(unconfirmed[i])
        for i in u_unc:
            unconfirmed[i].state = REMOVED
            self.removed_ids.add(unconfirmed[i].tid)
            self.branches["unconfirmed_removed"] += 1
        # new tracks
        live = {t.tid for t in self.tracked if t.state == TRACKED} | {t.tid for t in self.lost} | \
               {t.tid for t in lost_now if t.tid not in self.removed_ids}
        expired_ids = set()
        for j in u_det:
            d = dets[j]
            self._cmp([d.score], cfg["new_track_thresh"])
            if d.score < F32(cfg["new_track_thresh"]):
                self.branches["below_new_thresh"] += 1
                continue
            if len(live) >= self.max_tracks:
                self.overflow += 1
                self.branches["overflow"] += 1
                continue
            self.next_id += 1
            d.tid = self.next_id
            d.mean, d.cov = kf_initiate(tlwh_xyah(d.tlwh32))
            d.tlen, d.state, d.activated = 0, TRACKED, self.frame_id == 1
            d.frame = d.start = self.frame_id
            live.add(d.tid)
            activated.append(d)
            self.branches["new"] += 1
        # lists
        for t in self.lost:
            if self.frame_id - t.frame > self.max_time_lost:
                if t.state == LOST:
                    self.branches["expired"] += 1
                t.state = REMOVED
                expired_ids.add(t.tid)
        have = {t.tid for t in self.tracked if t.state == TRACKED}
        self.tracked = [t for t in self.tracked if t.state == TRACKED]
        for t in activated + refind:
            if t.tid not in have:
                have.add(t.tid)
                self.tracked.append(t)
        self.lost = [t for t in self.lost if t.tid not in have] + lost_now
        self.branches["lost_dropped"] += sum(t.tid in self.removed_ids for t in lost_now)
        self.lost = [t for t in self.lost if t.tid not in self.removed_ids]  # with the list of the frames before
        # remove_duplicate_stracks
        pd = iou_distance([t.xyxy for t in self.tracked], [t.xyxy for t in self.lost])
        self._cmp(pd, 0.15)
        dupa, dupb = set(), set()
        for p, q in zip(*np.where(pd < F32(0.15))):
            if self.tracked[p].age() > self.lost[q].age():
                dupb.add(int(q))
                self.branches["duplicate_lost_removed"] += 1
            else:
                dupa.add(int(p))
                self.branches["duplicate_tracked_removed"] += 1
        self.tracked = [t for i, t in enumerate(self.tracked) if i not in dupa]
        self.lost = [t for i, t in enumerate(self.lost) if i not in dupb]
        self.removed_ids |= expired_ids
        rows = [list(t.xyxy) + [t.tid, t.score, t.cls, t.idx] for t in self.tracked if t.activated]
        return np.asarray(rows, dtype=F32).reshape(-1, 8)


def run_sequence(frames, hw, cfg=None, reset_each=False, max_tracks=512, tracker=None):
    """The reference's per-image driver over `frames` (a list of [n_i, 6] fp32 arrays) through ONE tracker.
    -> (tracker, results); results[i] = (tracked flag, rows [k, 7] clipped to hw = (h, w), idx [k])."""
    trk = tracker or RefTracker(cfg, max_tracks)
    out = []
    for det in frames:
        if reset_each:
            trk.reset()
        det = np.asarray(det, dtype=F32).reshape(-1, 6)
        if len(det) == 0:
            trk.branches["empty_frame"] += 1
            out.append((0, np.zeros((0, 7), F32), np.zeros(0, int)))
            continue
        rows = trk.update(det)
        if len(rows) == 0:
            out.append((0, np.zeros((0, 7), F32), np.zeros(0, int)))
            continue
        b = rows[:, :7].copy()
        b[:, [0, 2]] = b[:, [0, 2]].clip(0, hw[1])
        b[:, [1, 3]] = b[:, [1, 3]].clip(0, hw[0])
        out.append((1, b, rows[:, 7].astype(int)))
    return trk, out


# ------------------------------------------------------------------------------------------ scenes
CANVAS = (256, 320)  # (h, w)


def _frame(boxes):
    """[(cx, cy, w, h, score, cls), ...] -> [n, 6] fp32 xyxy rows in descending score order (as an NMS emits them)."""
    rows = [[cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, s, c] for cx, cy, w, h, s, c in boxes]
    rows.sort(key=lambda r: -r[4])
    return np.asarray(rows, dtype=F32).reshape(-1, 6)


def scene_main(seed=0, frames=48):
    """6 objects in separate lanes moving linearly with jitter: one hidden for 4 frames (lost, re-found), one that
    leaves for good (expires: track_buffer 10), one entering late (unconfirmed, confirmed), one dropping to score
    0.12-0.22 for some frames (second association), one-frame false positives (unconfirmed, removed), an empty
    frame."""
    rng = np.random.default_rng(seed)
    lanes = [28, 68, 108, 148, 188, 228]
    x0 = rng.uniform(40, 90, 6)
    vx = rng.uniform(1.5, 3.0, 6)
    wh = rng.uniform(28, 34, (6, 2)) * [1.4, 1.0]
    out = []
    for f in range(frames):
        boxes = []
        if f == 40:
            out.append(_frame([]))
            continue
        for k in range(6):
            if k == 1 and 12 <= f < 16:
                continue
            if k == 2 and f >= 20:
                continue
            if k == 3 and f < 8:
                continue
            s = rng.uniform(0.12, 0.22) if (k == 4 and 24 <= f < 30) else rng.uniform(0.55, 0.9)
            jit = rng.uniform(-0.5, 0.5, 4)
            boxes.append((x0[k] + vx[k] * f + jit[0], lanes[k] + jit[1], wh[k, 0] + jit[2], wh[k, 1] + jit[3], s, k % 3))
        if f in (5, 18, 33):  # a one-frame false positive in the gap left of the lanes' traffic
            boxes.append((300.0, 40.0 + 60.0 * (f % 3), 24.0, 20.0, rng.uniform(0.4, 0.5), 1))
        out.append(_frame(boxes))
    return out, {"track_buffer": 10}


def scene_duplicates(seed=0):
    """match_thresh 0.6.  Top: a still object tracked 10 frames, then one frame at score 0.35 -- the fused cost
    passes 0.6, the track is lost and a new one starts on top of it (the younger tracked one is removed), then it is
    re-found.  Middle: a young track is lost where it stood; an old tracked object drives over the spot (the younger
    lost one is removed)."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(26):
        boxes = []
        j = rng.uniform(-0.15, 0.15, 8)
        boxes.append((60 + j[0], 40 + j[1], 50 + j[2], 40 + j[3], 0.35 if f == 10 else rng.uniform(0.75, 0.9), 0))
        boxes.append((43 + 6.0 * f + j[4], 150 + j[5], 60, 60, rng.uniform(0.75, 0.9), 1))  # the old mover
        if 1 <= f < 3:
            boxes.append((160 + j[6], 150 + j[7], 60, 60, rng.uniform(0.75, 0.9), 2))  # the young one, lost at f = 3
        out.append(_frame(boxes))
    return out, {"match_thresh": 0.6}


def scene_new_thresh(seed=0):
    """new_track_thresh 0.6: an object at score 0.4 is a high detection yet never starts a track."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(6):
        j = rng.uniform(-0.3, 0.3, 4)
        out.append(_frame([(80 + 2 * f + j[0], 60 + j[1], 40, 40, rng.uniform(0.7, 0.9), 0),
                           (200 + j[2], 180 + j[3], 40, 40, rng.uniform(0.38, 0.45), 1)]))
    return out, {"new_track_thresh": 0.6}


def scene_crossing(seed=0):
    """Two overlapping still objects, then one frame where both jump left so that the cheapest pair (track A, the
    detection between them) is not part of the optimum: greedy-by-lowest-cost differs from the assignment."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(8):
        j = rng.uniform(-0.1, 0.1, 4)
        ax, bx = (80.0, 112.0) if f == 6 else (100.0, 130.0)
        out.append(_frame([(ax + j[0], 100 + j[1], 60, 60, 0.9, 0), (bx + j[2], 100 + j[3], 60, 60, 0.88, 1)]))
    return out, {}


def scene_shapes(seed=0):
    """0, 1 and 2 detections; more tracks than detections and the reverse."""
    rng = np.random.default_rng(seed)
    spots = [(40 + 55 * k, 60 + 25 * (k % 3)) for k in range(5)] + [(60, 200), (200, 200)]
    show = [[0, 1, 2, 3, 4], [1, 3], [0, 1, 2, 3, 4, 5, 6], [], [2], [0, 5], [0, 1, 2, 3, 4, 5, 6], [6]]
    out = []
    for f, ks in enumerate(show):
        out.append(_frame([(spots[k][0] + f + rng.uniform(-0.3, 0.3), spots[k][1] + rng.uniform(-0.3, 0.3), 36, 30,
                            rng.uniform(0.5, 0.9), k % 3) for k in ks]))
    return out, {}


def scene_grid(seed=0):
    """300 detections: a 20 x 15 grid of 10 px boxes, uniform motion of 1 px per frame, 3 frames."""
    rng = np.random.default_rng(seed)
    score = rng.uniform(0.5, 0.9, 300)
    out = []
    for f in range(3):
        out.append(_frame([(9 + 16 * (k % 20) + f, 9 + 16 * (k // 20), 10, 10, score[k], k % 3) for k in range(300)]))
    return out, {}


def scene_zombie(seed=0):
    """track_buffer 2.  The reference marks a lost track removed once it is past max_time_lost but keeps it in
    lost_stracks for one more frame: here the object returns in exactly that frame and is re-found; its id now sits
    in removed_stracks, so when it is lost again it leaves the lost list at once, and its next return is a new id."""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(16):
        j = rng.uniform(-0.2, 0.2, 4)
        boxes = [(60 + j[0], 60 + j[1], 44, 36, rng.uniform(0.6, 0.9), 0)]
        if f < 4 or 7 <= f < 10 or f >= 12:
            boxes.append((200 + j[2], 150 + j[3], 40, 40, rng.uniform(0.6, 0.9), 1))
        out.append(_frame(boxes))
    return out, {"track_buffer": 2}


def scene_overflow():
    """12 separate detections in one frame, for max_tracks 8."""
    return [_frame([(20 + 25 * k, 50 + 10 * (k % 4), 20, 20, 0.9 - 0.02 * k, 0) for k in range(12)])], {}


def scene_nonfinite(seed=0):
    """scene_shapes' kind of traffic with a NaN box and an infinite box among the detections of two frames."""
    frames, cfg = scene_shapes(seed)
    frames = [f.copy() for f in frames]
    bad = np.array([[np.nan, 10, 50, 40, 0.8, 0], [10, 10, np.inf, 40, 0.7, 1]], dtype=F32)
    frames[1] = np.concatenate([bad[:1], frames[1]])
    frames[2] = np.concatenate([frames[2][:3], bad[1:], frames[2][3:]])
    return frames, cfg


SCENES = {
    "main0": lambda: scene_main(0), "main1": lambda: scene_main(1), "main2": lambda: scene_main(2),
    "main3": lambda: scene_main(3), "duplicates": scene_duplicates, "new_thresh": scene_new_thresh,
    "crossing": scene_crossing, "shapes": scene_shapes, "grid": scene_grid, "zombie": scene_zombie,
}
REQUIRED_BRANCHES = ["first_match", "second_match", "lost", "refind", "confirm", "unconfirmed_removed", "new",
                     "expired", "empty_frame", "duplicate_tracked_removed", "duplicate_lost_removed",
                     "below_new_thresh", "refind_removed", "lost_dropped"]


# ------------------------------------------------------------------------------------------ the device side
def gpu_track(frames, hw, cfg=None, *, mode="per_frame", reset_each=False, max_tracks=512, max_det=None,
              det_stride=0, graph=False, guard=False):
    """Feed `frames` through ydbl_bytetrack_update.  mode: "per_frame" (one call per frame, n = 1), "batch" (one
    call, n = len(frames), trackers = 1).  det_stride > 0: the detections lie in records of that many floats with
    the count in the record (as ydbl_nms writes them for a gathered batch).  graph: capture one update and replay it
    per frame over a refilled input buffer.  -> (results as run_sequence, header dict, extra)."""
    import ctypes as C

    import torch

    from ydbl import _lib

    cfg = {**CFG, **(cfg or {})}
    dev = torch.device("cuda")
    nf = len(frames)
    D = max_det or max(1, max(len(f) for f in frames))
    n = nf if mode == "batch" else 1
    rec = det_stride or D * 6
    cstride = rec if det_stride else 1
    buf = torch.zeros(n * rec + (0 if det_stride else n), dtype=torch.float32, device=dev)
    host = np.zeros(buf.numel(), dtype=F32)
    sbytes = int(_lib.lib.ydbl_bytetrack_state_bytes(max_tracks, D))
    pad = 4096 if guard else 0
    state = torch.zeros(sbytes + pad, dtype=torch.uint8, device=dev)
    if guard:
        state[sbytes:] = 0xA5
    out = torch.empty(n, D, 7, dtype=torch.float32, device=dev)
    oc = torch.empty(n, dtype=torch.int32, device=dev)
    tr = torch.empty(n, dtype=torch.int32, device=dev)
    oi = torch.empty(n, D, dtype=torch.int32, device=dev)
    hwt = torch.tensor([list(hw)] * n, dtype=torch.float32, device=dev)
    cnt_ptr = buf.data_ptr() + 4 * (D * 6 if det_stride else n * rec)
    d = _lib.TrackDesc(det=buf.data_ptr(), det_count=cnt_ptr, n=n, max_det=D, det_stride=det_stride,
                       count_stride=cstride if det_stride else 0, hw=hwt.data_ptr(),
                       track_high_thresh=cfg["track_high_thresh"], track_low_thresh=cfg["track_low_thresh"],
                       new_track_thresh=cfg["new_track_thresh"], match_thresh=cfg["match_thresh"],
                       fuse_score=int(cfg["fuse_score"]), track_buffer=cfg["track_buffer"],
                       max_time_lost=int(30 / 30.0 * cfg["track_buffer"]), max_tracks=max_tracks, trackers=1,
                       reset_each=int(reset_each), out=out.data_ptr(), out_count=oc.data_ptr(), tracked=tr.data_ptr(),
                       out_idx=oi.data_ptr(), state=state.data_ptr(), state_bytes=sbytes)

    def fill(group):
        host[:] = 0
        cview = host.view(np.int32)
        for i, f in enumerate(group):
            f = np.asarray(f, dtype=F32).reshape(-1, 6)
            host[i * rec: i * rec + f.size] = f.ravel()
            cview[(i * rec + D * 6) if det_stride else (n * rec + i)] = len(f)
        buf.copy_(torch.from_numpy(host))

    def collect(res):
        o, c, t, ix = out.cpu().numpy(), oc.cpu().numpy(), tr.cpu().numpy(), oi.cpu().numpy()
        for i in range(n):
            res.append((int(t[i]), o[i, : c[i]].copy(), ix[i, : c[i]].astype(int).copy()))
            assert not o[i, c[i]:].any() and (ix[i, c[i]:] == -1).all(), "rows past the count must be cleared"

    res = []
    stream = torch.cuda.current_stream()
    if mode == "batch":
        fill(frames)
        _lib.check(_lib.lib.ydbl_bytetrack_update(C.byref(d), stream.cuda_stream), "bytetrack")
        collect(res)
    elif graph:
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        fill(frames[:1])
        state_zero = state.clone()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                _lib.check(_lib.lib.ydbl_bytetrack_update(C.byref(d), side.cuda_stream), "bytetrack")
        torch.cuda.synchronize()
        state.copy_(state_zero)  # capture does not run the kernel; start from the zeroed state either way
        for f in frames:
            fill([f])
            g.replay()
            collect(res)
    else:
        for f in frames:
            fill([f])
            _lib.check(_lib.lib.ydbl_bytetrack_update(C.byref(d), stream.cuda_stream), "bytetrack")
            collect(res)
    torch.cuda.synchronize()
    raw = state.cpu().numpy()
    head = raw[:32].view(np.int32)
    header = {"frame_id": int(head[2]), "next_id": int(head[3]), "overflow": int(head[4]), "hwm": int(head[5])}
    return res, header, {"guard_ok": bool((raw[sbytes:] == 0xA5).all()) if guard else None}
