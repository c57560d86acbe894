"""ydbl_bytetrack_update on the MI355X, through the C-ABI, against the numpy restatement (tests/track_util.py).

Exactly equal: tracked, out_count, ids, cls, detection idx, row order, scores (bit-equal), frame_id / next id.
Boxes: fp64 filter on both sides, fp32 outputs.  Measured on the MI355X over every scene here:
max |box_gpu - box_restatement| = 0 px -- every output box is bit-equal after the rounding to fp32.  Four times the
measured value is 0, which would assert that the two fp64 filters never round a coordinate to different fp32
neighbours; their 8x8 products are summed in different orders, so they differ in the last fp64 bits and one such
flip is legitimate.  The bound is therefore one fp32 spacing at the canvas's largest coordinates (2^-15 = 3.05e-5 px
for 256 <= x < 512), rounded up to one digit: 4e-5 px -- from the number formats, not from the code under test, and
25 times below the 1e-3 px cap.
"""

import numpy as np
import pytest

import track_util as tu

pytestmark = pytest.mark.gpu

BOX_MEASURED = 0.0
BOX_TOL = 4e-5  # one fp32 spacing at 256 .. 512 px, rounded up to one digit
assert BOX_TOL <= 1e-3


def compare(got, want, what=""):
    """Exact equality of everything but the boxes; -> the largest box difference."""
    assert len(got) == len(want), what
    worst = 0.0
    for f, ((gt, gb, gi), (wt, wb, wi)) in enumerate(zip(got, want)):
        where = f"{what} frame {f}"
        assert gt == wt, where
        assert len(gb) == len(wb), where
        assert np.array_equal(gi, wi), where
        assert np.array_equal(gb[:, 4], wb[:, 4]), where                                    # ids, in order
        assert np.array_equal(gb[:, 5].view(np.int32), wb[:, 5].view(np.int32)), where      # scores bit-equal
        assert np.array_equal(gb[:, 6], wb[:, 6]), where                                    # cls
        if len(gb):
            worst = max(worst, float(np.abs(gb[:, :4].astype(np.float64) - wb[:, :4]).max()))
    return worst


@pytest.fixture(scope="module")
def reference():
    """name -> (frames, cfg, tracker, results) of the restatement, computed once."""
    out = {}
    for name, mk in tu.SCENES.items():
        frames, cfg = mk()
        trk, res = tu.run_sequence(frames, tu.CANVAS, cfg)
        out[name] = (frames, cfg, trk, res)
    return out


@pytest.mark.parametrize("name", list(tu.SCENES))
def test_scene_frame_by_frame_and_as_one_batch(reference, name):
    frames, cfg, trk, want = reference[name]
    D = 300 if name == "grid" else None
    got, head, _ = tu.gpu_track(frames, tu.CANVAS, cfg, max_det=D)
    worst = compare(got, want, name)
    assert head["frame_id"] == trk.frame_id and head["next_id"] == trk.next_id and head["overflow"] == 0
    got_b, head_b, _ = tu.gpu_track(frames, tu.CANVAS, cfg, mode="batch", max_det=D)
    worst = max(worst, compare(got_b, want, name + " (batch walk)"))
    assert head_b == head
    for a, b in zip(got, got_b):  # the walk over the batch is the same arithmetic: bit-equal
        assert np.array_equal(a[1], b[1])
    print(f"track scene {name}: max |box_gpu - box_ref| = {worst:.3g} px (asserted {BOX_TOL:g})")
    assert worst <= BOX_TOL


def test_reset_each_gives_ids_from_one_all_activated(reference):
    frames, cfg, _, _ = reference["shapes"]
    _, want = tu.run_sequence(frames, tu.CANVAS, cfg, reset_each=True)
    for mode in ("per_frame", "batch"):
        got, _, _ = tu.gpu_track(frames, tu.CANVAS, cfg, mode=mode, reset_each=True)
        assert compare(got, want, "reset_each " + mode) <= BOX_TOL
        for f, (_, rows, _) in zip(frames, got):
            assert len(rows) == len(f) and sorted(rows[:, 4].tolist()) == list(range(1, len(f) + 1))


def test_one_tracker_per_row(reference):
    """trackers == n: three rows fed different scenes, each equal to its own single-tracker run."""
    import ctypes as C

    import torch

    from ydbl import _lib

    names = ["main0", "duplicates", "crossing"]
    scenes = [reference[k] for k in names]
    cfg = {**tu.CFG, "track_buffer": 10, "match_thresh": 0.8}
    solo = [tu.gpu_track(s[0], tu.CANVAS, cfg, max_det=8)[0] for s in scenes]
    steps = max(len(s[0]) for s in scenes)
    n, D, T = 3, 8, 64
    dev = torch.device("cuda")
    det = torch.zeros(n, D, 6, device=dev)
    cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    sbytes = int(_lib.lib.ydbl_bytetrack_state_bytes(T, D))
    state = torch.zeros(n * sbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(n, D, 7, device=dev)
    oc, tr = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    hw = torch.tensor([list(tu.CANVAS)] * n, dtype=torch.float32, device=dev)
    d = _lib.TrackDesc(det=det.data_ptr(), det_count=cnt.data_ptr(), n=n, max_det=D, hw=hw.data_ptr(),
                       track_high_thresh=cfg["track_high_thresh"], track_low_thresh=cfg["track_low_thresh"],
                       new_track_thresh=cfg["new_track_thresh"], match_thresh=cfg["match_thresh"], fuse_score=1,
                       track_buffer=10, max_time_lost=10, max_tracks=T, trackers=n, out=out.data_ptr(),
                       out_count=oc.data_ptr(), tracked=tr.data_ptr(), state=state.data_ptr(),
                       state_bytes=n * sbytes)
    for f in range(steps):
        h = np.zeros((n, D, 6), np.float32)
        c = np.zeros(n, np.int32)
        for i, s in enumerate(scenes):
            if f < len(s[0]):
                c[i] = len(s[0][f])
                h[i, : c[i]] = s[0][f]
        det.copy_(torch.from_numpy(h))
        cnt.copy_(torch.from_numpy(c))
        _lib.check(_lib.lib.ydbl_bytetrack_update(C.byref(d), torch.cuda.current_stream().cuda_stream))
        o, k, t = out.cpu().numpy(), oc.cpu().numpy(), tr.cpu().numpy()
        for i, s in enumerate(scenes):
            if f < len(s[0]):
                assert t[i] == solo[i][f][0] and np.array_equal(o[i, : k[i]], solo[i][f][1]), (names[i], f)
            else:
                assert t[i] == 0 and k[i] == 0


def test_record_strides(reference):
    """The detections read out of [max_det * 6 floats | count | pad] records, as a gathered ydbl_nms writes them."""
    frames, cfg, _, want = reference["shapes"]
    D = 7
    for mode in ("per_frame", "batch"):
        got, _, _ = tu.gpu_track(frames, tu.CANVAS, cfg, mode=mode, max_det=D, det_stride=D * 6 + 4)
        assert compare(got, want, "strided " + mode) <= BOX_TOL


def test_max_tracks_overflow_starts_no_track_and_overwrites_nothing():
    frames, cfg = tu.scene_overflow()
    trk, want = tu.run_sequence(frames, tu.CANVAS, cfg, max_tracks=8)
    got, head, extra = tu.gpu_track(frames, tu.CANVAS, cfg, max_tracks=8, guard=True)
    assert compare(got, want, "overflow") <= BOX_TOL
    assert len(got[0][1]) == 8 and got[0][1][:, 4].tolist() == list(range(1, 9))
    assert head["overflow"] == 4 == trk.overflow and head["next_id"] == 8 and head["hwm"] == 8
    assert extra["guard_ok"], "bytes past ydbl_bytetrack_state_bytes were written"


def test_sizes_past_64_kib_of_lds(reference):
    """max_tracks 1024 with max_det 300 needs 104 KiB of LDS: the launch raises the kernel's dynamic limit first."""
    frames, cfg, trk, want = reference["shapes"]
    got, head, _ = tu.gpu_track(frames, tu.CANVAS, cfg, max_tracks=1024, max_det=300)
    assert compare(got, want, "1024 tracks") <= BOX_TOL
    assert head["next_id"] == trk.next_id and head["frame_id"] == trk.frame_id


def test_non_finite_detections_take_no_part():
    frames, cfg = tu.scene_nonfinite()
    trk, want = tu.run_sequence(frames, tu.CANVAS, cfg)
    got, head, _ = tu.gpu_track(frames, tu.CANVAS, cfg)
    assert compare(got, want, "nonfinite") <= BOX_TOL
    assert head["next_id"] == trk.next_id
    for _, rows, _ in got:
        assert np.isfinite(rows).all()
    clean, _ = tu.scene_shapes()
    ids = lambda res: [r[1][:, 4].tolist() for r in res]  # noqa: E731
    assert ids(got) == ids(tu.run_sequence(clean, tu.CANVAS, cfg)[1])  # as if those detections were not there


def test_graph_replay_equals_eager(reference):
    frames, cfg, _, _ = reference["main1"]
    eager, head, _ = tu.gpu_track(frames, tu.CANVAS, cfg)
    replay, head_g, _ = tu.gpu_track(frames, tu.CANVAS, cfg, graph=True)
    assert head == head_g
    for a, b in zip(eager, replay):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
