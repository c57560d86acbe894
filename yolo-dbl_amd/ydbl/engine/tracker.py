"""ByteTrack for ``Model.track``: settings, the device state, and the launch of ``ydbl_bytetrack_update``.

The association runs on the device behind the NMS, on the same stream, reading the session's ``det | count`` where
they lie (include/ydbl.h, csrc/track.hip); this module holds what stays on the host: the settings of
U/cfg/trackers/bytetrack.yaml restated as ``DEFAULTS`` (as engine.model.DEFAULTS restates default.yaml), their
validation, and the caller-owned state buffer.
"""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import torch

# U/cfg/trackers/bytetrack.yaml
DEFAULTS = {"tracker_type": "bytetrack", "track_high_thresh": 0.25, "track_low_thresh": 0.1, "new_track_thresh": 0.25,
            "track_buffer": 30, "match_thresh": 0.8, "fuse_score": True}
MAX_TRACKS = 512   # live tracks (tracked + lost + unconfirmed) per tracker
FRAME_RATE = 30    # U/trackers/track.py:45
TRACK_ROWS = ("sequence", "parallel")
_THRESHOLDS = ("track_high_thresh", "track_low_thresh", "new_track_thresh", "match_thresh")


def load_settings(tracker="bytetrack.yaml") -> dict:
    """The tracker settings from ``tracker``: the name ``bytetrack.yaml`` (the built-in DEFAULTS), a path to a YAML
    file of the reference's layout, or a dict.  ValueError for unknown keys, missing keys, an unknown tracker_type, a
    threshold outside [0, 1] or a negative track_buffer; NotImplementedError for ``tracker_type: botsort`` (its
    global motion compensation needs cv2's sparse optical flow)."""
    if isinstance(tracker, dict):
        cfg = dict(tracker)
    elif isinstance(tracker, (str, Path)):
        name = str(tracker)
        if name in ("bytetrack.yaml", "bytetrack"):
            cfg = dict(DEFAULTS)
        elif name in ("botsort.yaml", "botsort"):
            raise NotImplementedError("tracker 'botsort' is not implemented (its GMC needs cv2's sparse optical "
                                      "flow); use the default, 'bytetrack.yaml'")
        else:
            import yaml

            p = Path(name)
            if not p.is_file():
                raise ValueError(f"tracker settings file not found: {name}")
            cfg = yaml.safe_load(p.read_text())
            if not isinstance(cfg, dict):
                raise ValueError(f"{name} does not hold a mapping of tracker settings")
    else:
        raise ValueError(f"tracker must be a name, a YAML path or a dict, got {type(tracker).__name__}")
    kind = cfg.get("tracker_type")
    if kind == "botsort":
        raise NotImplementedError("tracker_type 'botsort' is not implemented (its GMC needs cv2's sparse optical "
                                  "flow); use tracker_type 'bytetrack'")
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"unknown tracker settings {unknown}; ByteTrack takes {sorted(DEFAULTS)}")
    missing = sorted(set(DEFAULTS) - set(cfg))
    if missing:
        raise ValueError(f"tracker settings are missing {missing}")
    if kind != "bytetrack":
        raise ValueError(f"tracker_type must be 'bytetrack', got {kind!r}")
    for k in _THRESHOLDS:
        v = cfg[k]
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"tracker setting {k} must be a number in [0, 1], got {v!r}")
        cfg[k] = float(v)
    tb = cfg["track_buffer"]
    if isinstance(tb, bool) or not isinstance(tb, int) or tb < 0:
        raise ValueError(f"tracker setting track_buffer must be an integer >= 0, got {tb!r}")
    if not isinstance(cfg["fuse_score"], bool):
        raise ValueError(f"tracker setting fuse_score must be a bool, got {cfg['fuse_score']!r}")
    return cfg


def settings_key(cfg: dict) -> tuple:
    return tuple(cfg[k] for k in sorted(DEFAULTS))


def max_time_lost(cfg: dict) -> int:
    return int(FRAME_RATE / 30.0 * cfg["track_buffer"])  # byte_tracker.py:289


def check_track_args(embed=None, track_rows="sequence", persist=False):
    """track()'s guards, before any device work."""
    if embed is not None and not (isinstance(embed, (list, tuple)) and not embed):
        raise ValueError("embed with track(): an embedding run returns no boxes to track; call embed() or predict()")
    if track_rows not in TRACK_ROWS:
        raise ValueError(f"track_rows must be one of {TRACK_ROWS}, got {track_rows!r}")
    if track_rows == "parallel" and not persist:
        raise ValueError("track_rows='parallel' needs persist=True: row i of every call is camera i's next frame")


class TrackerState:
    """The device state of `trackers` ByteTrack trackers (zeroed = reset) and the launch over a batch's records."""

    def __init__(self, cfg: dict, device, max_det: int, trackers: int = 1, max_tracks: int = MAX_TRACKS):
        from .. import _lib

        self._lib = _lib
        self.cfg, self.device = cfg, device
        self.max_det, self.trackers, self.max_tracks = int(max_det), int(trackers), int(max_tracks)
        self.bytes_per = int(_lib.lib.ydbl_bytetrack_state_bytes(self.max_tracks, self.max_det))
        if self.bytes_per <= 0:
            raise ValueError(f"bad tracker sizes: max_tracks {max_tracks}, max_det {max_det}")
        self.buf = torch.zeros(self.trackers * self.bytes_per, dtype=torch.uint8, device=device)
        self._words = self.buf.view(torch.int32).view(self.trackers, self.bytes_per // 4)
        self.overflow_seen = 0
        self._hw = {}

    def reset(self):
        self.buf.zero_()
        self.overflow_seen = 0

    def header(self):
        """Per tracker (frame_id, ids issued, overflow) -- one host sync."""
        return [tuple(r[2:5]) for r in self._words[:, :8].tolist()]

    def overflow(self) -> torch.Tensor:
        """The trackers' summed overflow counter, a 0-dim int32 device tensor (no sync)."""
        return self._words[:, 4].sum(dtype=torch.int32)

    def hw_tensor(self, shapes):
        key = tuple(shapes)
        t = self._hw.get(key)
        if t is None:
            if len(self._hw) > 16:
                self._hw.clear()
            t = self._hw[key] = torch.tensor([list(map(float, s)) for s in key], dtype=torch.float32,
                                             device=self.device)
        return t

    def update(self, det: torch.Tensor, count: torch.Tensor, shapes, reset_each: bool, want_idx: bool = False):
        """Enqueue one ydbl_bytetrack_update on the current stream over det [n, max_det, 6] / count [n] (any row
        strides: a session's buffers are read in place).  shapes: each image's (h, w).  -> out [n, max_det, 7],
        out_count [n], tracked [n] (device tensors; nothing is synchronised); want_idx: also out_idx [n, max_det]
        int32, each track row's detection index (-1 past the count)."""
        n = det.shape[0]
        assert det.shape[1] == self.max_det and det.dtype == torch.float32 and count.dtype == torch.int32
        assert det.stride(2) == 1 and det.stride(1) == 6
        out = torch.empty((n, self.max_det, 7), dtype=torch.float32, device=self.device)
        oc = torch.empty(2 * n, dtype=torch.int32, device=self.device)
        hw = self.hw_tensor(shapes)
        idx = torch.empty((n, self.max_det), dtype=torch.int32, device=self.device) if want_idx else None
        cfg = self.cfg
        d = self._lib.TrackDesc(
            det=det.data_ptr(), det_count=count.data_ptr(), n=n, max_det=self.max_det, det_stride=det.stride(0),
            count_stride=count.stride(0), hw=hw.data_ptr(), track_high_thresh=cfg["track_high_thresh"],
            track_low_thresh=cfg["track_low_thresh"], new_track_thresh=cfg["new_track_thresh"],
            match_thresh=cfg["match_thresh"], fuse_score=int(cfg["fuse_score"]), track_buffer=cfg["track_buffer"],
            max_time_lost=max_time_lost(cfg), max_tracks=self.max_tracks, trackers=self.trackers,
            reset_each=int(bool(reset_each)), out=out.data_ptr(), out_count=oc.data_ptr(),
            tracked=oc.data_ptr() + 4 * n, out_idx=idx.data_ptr() if want_idx else None, state=self.buf.data_ptr(),
            state_bytes=self.buf.numel())
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self._lib.check(self._lib.lib.ydbl_bytetrack_update(C.byref(d), stream), "ydbl_bytetrack_update")
        return (out, oc[:n], oc[n:], idx) if want_idx else (out, oc[:n], oc[n:])

    def check_overflow(self, total: int):
        """Raise when the overflow counter moved since it was last looked at (a track could not be started)."""
        if total != self.overflow_seen:
            lost, self.overflow_seen = total - self.overflow_seen, total
            raise RuntimeError(f"tracker overflow: {lost} detection(s) could not start a track, more than max_tracks="
                               f"{self.max_tracks} tracks are alive (tracked + lost + unconfirmed); pass a larger "
                               "max_tracks to track() or a smaller track_buffer")


class LazyTracks:
    """A tracked batch's boxes, chosen on first access with ONE host sync: image i's rows are the tracker's 7-column
    rows when it produced any, else the predicted 6-column rows (U/trackers/track.py:78-87)."""

    def __init__(self, state: TrackerState, out, out_count, tracked, dets, counts):
        self.state, self.out, self.dets = state, out, dets
        self._dev = (out_count, tracked, counts, state.overflow())
        self.host = None

    def _sync(self):
        if self.host is None:
            oc, tr, cnt, ovf = self._dev
            n = oc.numel()
            flat = torch.cat([oc, tr, cnt, ovf.reshape(1)]).tolist()
            self.host = (flat[:n], flat[n:2 * n], flat[2 * n:3 * n])
            self._dev = None
            self.state.check_overflow(flat[-1])
        return self.host

    def __getitem__(self, i):
        oc, tr, cnt = self._sync()
        return self.out[i, : oc[i]] if tr[i] else self.dets[i, : cnt[i]]

    mask_src = None  # a segmentation model's track(): (i -> the image's predicted masks or None, out_idx)
    kpt_src = None  # a pose model's track(): (the batch's keypoints [n, max_det, K, ndim], out_idx)

    def keypoints(self, i):
        """Image i's keypoints in the order of its boxes: the predicted rows picked by the track rows' detection
        indices when the image got tracks (results[i][idx], U/trackers/track.py:83-84), else as predicted."""
        oc, tr, cnt = self._sync()
        kp, idx = self.kpt_src
        return kp[i][idx[i, : oc[i]].long()] if tr[i] else kp[i, : cnt[i]]

    def masks(self, i):
        """Image i's masks in the order of its boxes: the predicted masks picked by the track rows' detection indices
        when the image got tracks (results[i][idx], U/trackers/track.py:83-84), else as predicted; None without one."""
        oc, tr, _ = self._sync()
        fn, idx = self.mask_src
        m = fn(i)
        if m is None or not tr[i]:
            return m
        return m[idx[i, : oc[i]].long()]
