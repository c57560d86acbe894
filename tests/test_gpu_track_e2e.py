"""track() end to end on the MI355X: DBL-n, nc 3, the trained-like fixture, blob images at 128 x 128, fp32.  The
frames are one image translated by a few pixels per frame (torch.roll) -- as a tensor batch for the tensor path and
as uint8 HWC BGR frames for the frame path.  Every run is compared with the numpy restatement
(tests/track_util.py) fed with predict(**PRED)'s boxes for the same inputs: ids, order, the 7-column layout,
boxes.id / is_track, clipping to orig_shape; persist, reset_trackers(), track_rows="parallel".

The fixture's detector answers blob images with scores of 0.10 .. 0.27 and, class by class, near-copies of one box.
Left as it is that input has no unique assignment (tied costs) and nothing above ByteTrack's default 0.25, so both
sides run with agnostic NMS at IoU 0.3 (distinct boxes) and the tracker settings TRACKER below (score split at
0.1123, plain IoU cost: a fused cost of 1 - iou * 0.12 never passes 0.8).  Seeds and shifts were chosen for inputs
whose assignments are unique by a margin; every comparison asserts that condition on its own input first
(margin >= 1e-3, thresholds clear by 1e-4), as tests/test_track_host.py does for the synthetic scenes.

Box tolerance: one fp32 spacing at 64 .. 128 px (2^-17 = 7.6e-6 px), rounded up to one digit -- the reasoning of
tests/test_gpu_track.py at this canvas's coordinates."""

import numpy as np
import pytest
import torch

import track_util as tu

pytestmark = pytest.mark.gpu

S, NF = 128, 6
BOX_TOL = 8e-6
PRED = dict(conf=0.1, agnostic_nms=True, iou=0.3)
TRACKER = {**tu.CFG, "fuse_score": False, "track_high_thresh": 0.1123, "new_track_thresh": 0.1123}
TRACK = dict(tracker=TRACKER, agnostic_nms=True, iou=0.3)


def restate(preds, **kw):
    """The restatement over predicted boxes, with the input conditions asserted."""
    trk, want = tu.run_sequence(preds, (S, S), TRACKER, **kw)
    print("e2e input: detections", [len(p) for p in preds], "tracks", [len(w[1]) for w in want], "ids", trk.next_id,
          "margin", min(trk.margins) if trk.margins else None, "near", trk.near, dict(trk.branches))
    assert not trk.margins or min(trk.margins) >= 1e-3, "input condition: the assignment must be unique by a margin"
    assert trk.near >= 1e-4, "input condition: a threshold comparison is too close to its threshold"
    return trk, want


@pytest.fixture(scope="module")
def model(golden_dir):
    from ydbl import YOLO
    from ydbl.utils.synthetic import load_trained

    torch.manual_seed(0)
    m = YOLO("yolov13n_DBL.yaml", nc=3)
    load_trained(m.model, golden_dir / "trained_yolov13n_DBL_nc3.npz")
    return m


def rolled(seed, dx, dy):
    from ydbl.utils.synthetic import blob_images

    base = blob_images(1, S, seed=seed)[0]
    return torch.stack([torch.roll(base, shifts=(dy * k, dx * k), dims=(1, 2)) for k in range(NF)])


@pytest.fixture(scope="module")
def x():
    return rolled(42, -2, 3)


def boxes_of(results):
    return [r.boxes.data.cpu().numpy() for r in results]


def check(results, preds, want, tol=BOX_TOL):
    """Results of track() against the restatement's (flag, rows, idx) fed with the predicted boxes `preds`."""
    assert len(results) == len(want)
    for r, p, (flag, rows, idx) in zip(results, preds, want):
        data = r.boxes.data.cpu().numpy()
        if not flag:  # the Results stay as predicted
            assert not r.boxes.is_track and r.boxes.id is None and np.array_equal(data, p)
            continue
        assert data.shape == (len(rows), 7) and r.boxes.is_track
        assert np.array_equal(r.boxes.id.cpu().numpy(), rows[:, 4])
        assert np.array_equal(data[:, 5:], p[idx][:, 4:6])  # conf, cls of the matched detections, bit-equal
        assert np.array_equal(data[:, 4:], rows[:, 4:7])
        assert np.abs(data[:, :4].astype(np.float64) - rows[:, :4]).max() <= tol
        h, w = r.orig_shape
        assert data[:, [0, 2]].min() >= 0 and data[:, [0, 2]].max() <= w
        assert data[:, [1, 3]].min() >= 0 and data[:, [1, 3]].max() <= h
        assert np.array_equal(r.boxes.conf.cpu().numpy(), data[:, 5]) and np.array_equal(r.boxes.cls.cpu().numpy(), data[:, 6])


def ids_of(results):
    return [None if r.boxes.id is None else r.boxes.id.cpu().tolist() for r in results]


def test_tensor_source_calls_of_one_and_one_batch(model, x):
    xg = x.cuda()
    before = boxes_of(model.predict(xg, **PRED))
    model.reset_trackers()
    seq = [model.track(xg[k: k + 1], persist=True, **TRACK)[0] for k in range(NF)]
    pred1 = [model.predict(xg[k: k + 1], **PRED)[0].boxes.data.cpu().numpy() for k in range(NF)]
    trk, want = restate(pred1)
    assert sum(len(w[1]) for w in want) >= NF, "the fixture must give tracks, or this test shows nothing"
    check(seq, pred1, want)
    assert model._trackers and next(iter(model._trackers.values())).header()[0][:2] == (trk.frame_id, trk.next_id)
    # the same frames as ONE call: the rows are consecutive frames of one tracker
    model.reset_trackers()
    one = model.track(xg, persist=True, **TRACK)
    check(one, before, restate(before)[1])
    assert ids_of(one) == ids_of(seq)
    # predict() is what it was: tracking leaves the session's results alone
    after = boxes_of(model.predict(xg, **PRED))
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert all(b.shape[1] == 6 for b in after)


def test_persist_false_resets_before_every_image(model, x):
    xg = x.cuda()
    pred = boxes_of(model.predict(xg, **PRED))
    res = model.track(xg, **TRACK)  # persist=False
    check(res, pred, restate(pred, reset_each=True)[1])
    for r, p in zip(res, pred):
        if len(p) and r.boxes.is_track:
            assert sorted(r.boxes.id.cpu().tolist()) == list(range(1, len(r.boxes) + 1))
    again = model.track(xg[:1], **TRACK)
    assert ids_of(again) == ids_of(res[:1])


def test_reset_trackers_and_persist_across_calls(model, x):
    xg = x.cuda()
    model.reset_trackers()
    a = model.track(xg[:3], persist=True, **TRACK)
    b = model.track(xg[3:], persist=True, **TRACK)
    model.reset_trackers()
    whole = model.track(xg, persist=True, **TRACK)
    assert ids_of(a) + ids_of(b) == ids_of(whole)  # persist carries the identities over the call boundary
    model.reset_sessions()  # weights and sessions do not invalidate identities
    model.track(xg[:1], persist=True, **TRACK)
    frame_c = next(iter(model._trackers.values())).header()[0][0]
    model.reset_trackers()
    d = model.track(xg[:1], persist=True, **TRACK)
    frame_d = next(iter(model._trackers.values())).header()[0][0]
    assert ids_of(d) == ids_of(whole[:1])
    assert frame_c > frame_d == 1  # the first went on with the old tracker, the second started a new one


def test_parallel_rows_are_independent_trackers(model, x):
    y = rolled(11, -2, 3)
    model.reset_trackers()
    got, preds = [[], []], [[], []]
    for k in range(4):
        pair = torch.stack([x[k], y[k]]).cuda()
        res = model.track(pair, persist=True, track_rows="parallel", **TRACK)
        pr = boxes_of(model.predict(pair, **PRED))
        for i in range(2):
            got[i].append(res[i])
            preds[i].append(pr[i])
    for i in range(2):
        check(got[i], preds[i], restate(preds[i])[1])  # ids per tracker, each counted from 1
    with pytest.raises(ValueError, match="parallel"):
        model.track(x[:3].cuda(), persist=True, track_rows="parallel", **TRACK)
    model.reset_trackers()


def test_frame_source_goes_through_the_same_kernel(model, x):
    frames = [np.ascontiguousarray((x[k] * 255).round().byte().permute(1, 2, 0).numpy()[..., ::-1]) for k in range(NF)]
    pred = boxes_of(model.predict(frames, **PRED, imgsz=S))
    model.reset_trackers()
    res = model.track(frames, persist=True, imgsz=S, **TRACK)
    trk, want = restate(pred)
    assert sum(len(w[1]) for w in want) >= NF
    check(res, pred, want)
    assert all(r.orig_shape == (S, S) for r in res)
    one_by_one = []
    model.reset_trackers()
    for f in frames:
        one_by_one += model.track(f, persist=True, imgsz=S, **TRACK)
    assert ids_of(one_by_one) == ids_of(res)
    model.reset_trackers()


def test_path_source_batches_walk_one_tracker(model, x, tmp_path):
    from PIL import Image

    frames = [np.ascontiguousarray((x[k] * 255).round().byte().permute(1, 2, 0).numpy()[..., ::-1]) for k in range(3)]
    for k, f in enumerate(frames):
        Image.fromarray(f[..., ::-1].copy()).save(tmp_path / f"f{k}.png")  # lossless: the same pixels as the frames
    model.reset_trackers()
    want = model.track(frames, persist=True, imgsz=S, **TRACK)
    model.reset_trackers()
    got = model.track(str(tmp_path), persist=True, batch=2, imgsz=S, **TRACK)  # batches of 2 and 1, one tracker
    assert len(got) == 3 and [r.path for r in got] == sorted(r.path for r in got)
    assert ids_of(got) == ids_of(want)
    assert all(np.array_equal(a, b) for a, b in zip(boxes_of(got), boxes_of(want)))
    fresh = model.track(str(tmp_path), batch=2, imgsz=S, **TRACK)  # persist=False: reset before every image
    assert all(r.boxes.id is None or sorted(r.boxes.id.cpu().tolist()) == list(range(1, len(r.boxes) + 1))
               for r in fresh)
    model.reset_trackers()


def test_overflow_raises_when_the_results_are_looked_at(model, x):
    xg = x[:1].cuda()
    n = len(model.predict(xg, **PRED)[0].boxes)
    assert n >= 2, "needs two detections in the first frame"
    res = model.track(xg, max_tracks=1, **TRACK)  # returns without a sync
    with pytest.raises(RuntimeError, match="max_tracks"):
        res[0].boxes
    model.reset_trackers()


def test_stream_and_results_helpers_with_ids(model, x, tmp_path):
    model.reset_trackers()
    it = model.track(x[:2].cuda(), persist=True, stream=True, **TRACK)
    assert not isinstance(it, list)
    res = list(it)
    r = next((r for r in res if r.boxes.is_track and len(r.boxes)), None)
    assert r is not None
    ids = [int(v) for v in r.boxes.id.cpu().tolist()]
    assert [d["track_id"] for d in r.summary()] == ids
    assert all(0 <= d["confidence"] <= 1 for d in r.summary())
    r.save_txt(tmp_path / "a.txt", save_conf=True)
    rows = [ln.split() for ln in (tmp_path / "a.txt").read_text().splitlines()]
    assert [int(v[-1]) for v in rows] == ids and all(len(v) == 7 for v in rows)
    assert r.plot().shape == (S, S, 3)
    model.reset_trackers()
