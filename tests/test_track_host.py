"""track() without a GPU: the tracker settings and their errors, track()'s guards, the C-ABI's argument validation,
and the conditions the GPU tests' inputs must meet (checked on the restatement alone, tests/track_util.py): every
named branch fires, every assignment is unique by a margin >= 1e-3, and no threshold comparison lies within 1e-4 of
its threshold.  If a seed violates them, change the seed, not the bound."""

import ctypes as C
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import track_util as tu

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------ settings
def test_builtin_settings_restate_bytetrack_yaml():
    from ydbl.engine.tracker import DEFAULTS, load_settings, max_time_lost

    cfg = load_settings("bytetrack.yaml")
    assert cfg == DEFAULTS == tu.CFG
    assert (cfg["track_high_thresh"], cfg["track_low_thresh"], cfg["new_track_thresh"], cfg["track_buffer"],
            cfg["match_thresh"], cfg["fuse_score"]) == (0.25, 0.1, 0.25, 30, 0.8, True)
    assert max_time_lost(cfg) == 30 and max_time_lost({**cfg, "track_buffer": 10}) == 10
    cfg["match_thresh"] = 0.5
    assert DEFAULTS["match_thresh"] == 0.8  # a copy


def test_settings_from_a_dict_and_from_a_yaml_file(tmp_path):
    from ydbl.engine.tracker import DEFAULTS, load_settings

    assert load_settings({**DEFAULTS, "track_buffer": 10})["track_buffer"] == 10
    p = tmp_path / "mine.yaml"
    p.write_text("tracker_type: bytetrack\ntrack_high_thresh: 0.3\ntrack_low_thresh: 0.05\nnew_track_thresh: 0.4\n"
                 "track_buffer: 12\nmatch_thresh: 0.7\nfuse_score: False\n")
    assert load_settings(str(p)) == {"tracker_type": "bytetrack", "track_high_thresh": 0.3, "track_low_thresh": 0.05,
                                     "new_track_thresh": 0.4, "track_buffer": 12, "match_thresh": 0.7,
                                     "fuse_score": False}
    assert load_settings(p)["track_buffer"] == 12


def test_settings_errors(tmp_path):
    from ydbl.engine.tracker import DEFAULTS, load_settings

    with pytest.raises(ValueError, match="unknown tracker settings"):
        load_settings({**DEFAULTS, "gmc_method": "sparseOptFlow"})
    with pytest.raises(ValueError, match="missing"):
        load_settings({k: v for k, v in DEFAULTS.items() if k != "match_thresh"})
    for k, bad in [("track_high_thresh", 1.5), ("track_low_thresh", -0.1), ("match_thresh", "0.8"),
                   ("new_track_thresh", float("nan")), ("track_buffer", -1), ("track_buffer", 2.5), ("fuse_score", 1)]:
        with pytest.raises(ValueError, match=k):
            load_settings({**DEFAULTS, k: bad})
    with pytest.raises(ValueError, match="tracker_type"):
        load_settings({**DEFAULTS, "tracker_type": "sort"})
    with pytest.raises(ValueError, match="not found"):
        load_settings(str(tmp_path / "nothing.yaml"))
    with pytest.raises(ValueError):
        load_settings(3)


def test_botsort_is_refused(tmp_path):
    from ydbl.engine.tracker import DEFAULTS, load_settings

    with pytest.raises(NotImplementedError, match="botsort"):
        load_settings("botsort.yaml")
    with pytest.raises(NotImplementedError, match="botsort"):
        load_settings({**DEFAULTS, "tracker_type": "botsort", "gmc_method": "sparseOptFlow"})
    p = tmp_path / "b.yaml"
    p.write_text("tracker_type: botsort\nwith_reid: False\n")
    with pytest.raises(NotImplementedError, match="botsort"):
        load_settings(str(p))


# ------------------------------------------------------------------------------------------ track()'s guards
@pytest.fixture(scope="module")
def model():
    from ydbl import YOLO

    return YOLO("yolov13n_DBL.yaml", nc=3)


def test_track_guards_raise_before_any_device_work(model):
    """Each of these is raised with no GPU present (select_device would raise RuntimeError after them)."""
    import torch

    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(ValueError, match="embed"):
        model.track(x, embed=[3])
    with pytest.raises(ValueError, match="track_rows"):
        model.track(x, track_rows="columns")
    with pytest.raises(ValueError, match="persist"):
        model.track(x, track_rows="parallel")
    with pytest.raises(NotImplementedError, match="botsort"):
        model.track(x, tracker="botsort.yaml")
    with pytest.raises(ValueError, match="unknown tracker settings"):
        model.track(x, tracker={**tu.CFG, "proximity_thresh": 0.5})
    with pytest.raises(ValueError, match="max_tracks"):
        model.track(x, max_tracks=0)
    with pytest.raises(ValueError, match="source"):
        model.track(None)
    with pytest.raises(TypeError, match="unsupported source"):
        model.track(3.5)
    assert model._trackers == {} and model.reset_trackers() is model


def test_track_signature_and_defaults():
    import inspect

    from ydbl import YOLO

    sig = inspect.signature(YOLO.track)
    assert [p for p in sig.parameters][1:] == ["source", "stream", "persist", "tracker", "track_rows", "kwargs"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["source"], d["stream"], d["persist"], d["tracker"], d["track_rows"]) == \
           (None, False, False, "bytetrack.yaml", "sequence")
    assert "botsort" in YOLO.track.__doc__ and "ByteTrack" in YOLO.track.__doc__


# ------------------------------------------------------------------------------------------ the C-ABI
def _desc(**over):
    from ydbl import _lib

    base = dict(det=0x1000, det_count=0x1000, n=2, max_det=8, hw=0x1000, track_high_thresh=0.25,
                track_low_thresh=0.1, new_track_thresh=0.25, match_thresh=0.8, fuse_score=1, track_buffer=30,
                max_time_lost=30, max_tracks=16, trackers=1, out=0x1000, out_count=0x1000, tracked=0x1000,
                state=0x1000, state_bytes=1 << 30)
    base.update(over)
    return _lib.TrackDesc(**base)


@pytest.mark.parametrize("over, word", [
    (dict(det=None), "null"), (dict(det_count=None), "null"), (dict(hw=None), "null"), (dict(out=None), "null"),
    (dict(out_count=None), "null"), (dict(tracked=None), "null"), (dict(state=None), "null"),
    (dict(trackers=3), "trackers"), (dict(trackers=0), "trackers"), (dict(max_tracks=0), "max_tracks"),
    (dict(max_tracks=-4), "max_tracks"), (dict(n=0), "n and max_det"), (dict(max_det=0), "n and max_det"),
    (dict(det_stride=47), "det_stride"), (dict(match_thresh=1.5), "thresholds"),
    (dict(track_high_thresh=float("nan")), "thresholds"), (dict(state_bytes=64), "state buffer"),
    (dict(state=0x1008), "aligned"), (dict(max_time_lost=-1), "max_time_lost"),
])
def test_update_rejects_bad_arguments_without_launching(over, word):
    from ydbl import _lib

    rc = _lib.lib.ydbl_bytetrack_update(C.byref(_desc(**over)), None)
    assert rc != 0
    assert word in _lib.lib.ydbl_last_error().decode()


def test_update_rejects_a_null_descriptor_and_sizes_beyond_the_lds():
    from ydbl import _lib

    assert _lib.lib.ydbl_bytetrack_update(None, None) != 0
    assert "null descriptor" in _lib.lib.ydbl_last_error().decode()
    assert _lib.lib.ydbl_bytetrack_update(C.byref(_desc(max_tracks=4096, max_det=300)), None) == 3  # YDBL_ECAPACITY
    assert "LDS" in _lib.lib.ydbl_last_error().decode()


def test_state_bytes_is_monotone():
    from ydbl import _lib

    f = _lib.lib.ydbl_bytetrack_state_bytes
    assert f(0, 300) == -1 and f(512, 0) == -1
    sizes = [[f(t, d) for d in (1, 8, 300, 1000)] for t in (1, 2, 8, 64, 512, 513)]
    for row in sizes:
        assert all(b >= a > 0 for a, b in zip(row, row[1:]))
    for a, b in zip(sizes, sizes[1:]):
        assert all(y > x for x, y in zip(a, b))
    assert f(512, 300) % 16 == 0 and f(512, 300) >= 512 * (8 + 64) * 8  # mean and covariance in fp64 per slot


def test_descriptor_layout_matches_c(tmp_path):
    from ydbl import _lib

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "ydbl.h"}"', "int main(void){",
             'printf("size %zu\\n", sizeof(ydbl_track_desc));']
    for name, _ in _lib.TrackDesc._fields_:
        lines.append(f'printf("{name} %zu\\n", offsetof(ydbl_track_desc, {name}));')
    lines.append("return 0;}")
    (tmp_path / "t.c").write_text("\n".join(lines))
    subprocess.run(["gcc", str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "t")], check=True, capture_output=True,
                                                   text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(_lib.TrackDesc)
    for name, _ in _lib.TrackDesc._fields_:
        assert int(got[name]) == getattr(_lib.TrackDesc, name).offset, name


# ------------------------------------------------------------------------------------------ the GPU tests' inputs
@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, mk in tu.SCENES.items():
        frames, cfg = mk()
        out[name] = tu.run_sequence(frames, tu.CANVAS, cfg)[0]
    return out


def test_every_named_branch_fires_across_the_scenes(runs):
    total = Counter()
    for trk in runs.values():
        total += trk.branches
    for b in tu.REQUIRED_BRANCHES:
        assert total[b] >= 1, b
    # where each scene is aimed
    for k in ("main0", "main1", "main2", "main3"):
        for b in ("second_match", "lost", "refind", "confirm", "unconfirmed_removed", "expired", "empty_frame"):
            assert runs[k].branches[b] >= 1, (k, b)
    assert runs["duplicates"].branches["duplicate_tracked_removed"] >= 1
    assert runs["duplicates"].branches["duplicate_lost_removed"] >= 1
    assert runs["new_thresh"].branches["below_new_thresh"] >= 1 and runs["new_thresh"].next_id == 1
    assert runs["zombie"].branches["refind_removed"] == 1 and runs["zombie"].branches["lost_dropped"] == 1
    assert runs["zombie"].next_id == 3  # the steady object, the returning one, and its new id after the drop
    assert runs["grid"].next_id == 300 and runs["grid"].branches["first_match"] == 600


@pytest.mark.parametrize("name", list(tu.SCENES))
def test_assignments_are_unique_by_a_margin_and_thresholds_are_clear(runs, name):
    trk = runs[name]
    assert trk.margins and min(trk.margins) >= 1e-3, min(trk.margins)
    assert trk.near >= 1e-4, trk.near


def test_the_other_gpu_inputs_meet_the_same_conditions():
    for frames, cfg, kw in [(*tu.scene_overflow(), dict(max_tracks=8)), (*tu.scene_nonfinite(), {}),
                            (*tu.scene_shapes(), dict(reset_each=True))]:
        trk = tu.run_sequence(frames, tu.CANVAS, cfg, **kw)[0]
        assert trk.near >= 1e-4 and (not trk.margins or min(trk.margins) >= 1e-3)
    assert tu.run_sequence(*tu.scene_overflow()[:1], tu.CANVAS, {}, max_tracks=8)[0].overflow == 4


def test_the_crossing_scene_defeats_greedy_matching(runs):
    differs = [(f, stage) for f, stage, cost, lim, pairs in runs["crossing"].costs
               if cost.size and tu.greedy_pairs(cost, lim) != pairs]
    assert differs, "no frame where greedy-by-lowest-cost differs from the optimum"


def test_assignment_is_the_optimum_of_the_limited_objective():
    """The restatement's solver against brute force over all partial matchings, on small random matrices."""
    import itertools

    rng = np.random.default_rng(5)
    for _ in range(60):
        n, m = rng.integers(1, 5, 2)
        cost = rng.uniform(0, 1.2, (n, m))
        lim = 0.8
        best = 0.0
        for k in range(1, min(n, m) + 1):
            for rows in itertools.combinations(range(n), k):
                for cols in itertools.permutations(range(m), k):
                    best = min(best, sum(cost[i, j] - lim for i, j in zip(rows, cols)))
        pairs, ur, uc, _ = tu.assignment(cost, lim)
        assert abs(sum(cost[i, j] - lim for i, j in pairs) - best) < 1e-12
        assert all(cost[i, j] <= lim for i, j in pairs)
        assert sorted(ur + [i for i, _ in pairs]) == list(range(n))
