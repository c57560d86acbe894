"""DetectSession without a decode pass (DBL-n, nc <= 4, fp16, no keep_pred): the class-conv tail launches emit the NMS
candidates (ydbl.engine.session, _fuse_candidates).  det / count / cand_count equal, bit for bit, those of a
keep_pred=True session of the same arguments, which keeps ydbl_detect_decode; and the sessions that must keep the
decode launch -- DBL-s (its class conv is a launch of its own), augment=True -- still do."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(cfg, golden_dir):
    from ydbl import YOLO
    from ydbl.utils.synthetic import load_trained

    scale = cfg[7]
    torch.manual_seed(0)
    p = YOLO(cfg, nc=3)
    load_trained(p.model, golden_dir / f"trained_yolov13{scale}_DBL_nc3.npz")
    return p


@pytest.fixture(scope="module")
def dbl_n(golden_dir):
    return _model("yolov13n_DBL.yaml", golden_dir)


def _step_names(sess):
    return [st.fn.__name__ for p in sess.plans for st in p.steps]


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("size", [64, 96])
def test_fused_session_equals_decode_session(dbl_n, size, streams):
    from ydbl.utils.synthetic import blob_images

    x = blob_images(3, size, seed=5).cuda()
    kw = dict(half=True, conf=0.05, streams=streams)
    fused = dbl_n.session(3, size, size, **kw)
    plain = dbl_n.session(3, size, size, keep_pred=True, **kw)
    assert "ydbl_detect_decode" not in _step_names(fused)
    assert _step_names(plain).count("ydbl_detect_decode") == len(plain.plans)
    d0, c0 = plain(x)
    torch.cuda.synchronize()
    d0, c0, n0 = d0.clone(), c0.clone(), plain.cand_count.clone()
    outs = []
    for _ in range(2):  # two replays of the captured graph: the counters are zeroed per call
        d, c = fused(x)
        torch.cuda.synchronize()
        outs.append((d.clone(), c.clone(), fused.cand_count.clone()))
    for d, c, n in outs:
        assert torch.equal(n, n0)
        assert torch.equal(c, c0) and torch.equal(d, d0)
    assert int(n0.sum()) > 0 and int(c0.sum()) > 0


def test_sessions_that_keep_the_decode_launch(dbl_n, golden_dir):
    s = _model("yolov13s_DBL.yaml", golden_dir).session(2, 64, 64, half=True, conf=0.05)
    assert _step_names(s).count("ydbl_detect_decode") == 1
    a = dbl_n.session(2, 64, 64, half=True, conf=0.05, augment=True)
    assert _step_names(a).count("ydbl_detect_decode_aug") == 3 and "ydbl_detect_decode" not in _step_names(a)
    f = dbl_n.session(2, 64, 64, half=False, conf=0.05)  # fp32: the decode launch stays
    assert _step_names(f).count("ydbl_detect_decode") == 1
