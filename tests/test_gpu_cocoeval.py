"""ydbl_coco_match on the MI355X through coco_batch: every output equal to the numpy restatement of the COCO protocol
(cocoeval_util.py) on seeded scenes — ranks, matched / ignored masks, label flags, invalid counts, array_equal —,
then the 12 stats and COCOeval's three arrays from those outputs to 1e-12, determinism and graph capture.  The
scenes' content is asserted in test_cocoeval_host.py (test_scenes_are_not_trivial)."""

import numpy as np
import pytest
import torch

import cocoeval_util as U

pytestmark = pytest.mark.gpu

TOL = 1e-12  # values in [0, 1], both sides fp64 sums of at most a few thousand terms
KEYS = ("rank", "matched", "ignored", "gt_ignore", "invalid")


def gpu_arrays(batch, nc, single, **kw):
    from ydbl.engine.validator import coco_batch

    det, cnt, boxes, cls, bidx = batch
    out = coco_batch(torch.from_numpy(det).cuda(), torch.from_numpy(cnt).cuda(), torch.from_numpy(boxes),
                     torch.from_numpy(cls), torch.from_numpy(bidx), nc, single, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def assert_arrays(got, want):
    assert got["rank"].dtype == torch.int32 and got["gt_ignore"].dtype == torch.uint8
    for k in KEYS:
        assert np.array_equal(got[k].numpy(), want[k]), k


def product_stats(batches, outs, nc, single):
    from ydbl.engine.validator import coco_host_record
    from ydbl.utils.metrics import coco_accumulate, coco_summarize

    recs = []
    for (det, cnt, boxes, cls, bidx), out in zip(batches, outs):
        by_image = np.argsort(bidx, kind="stable")
        recs.append(coco_host_record(torch.from_numpy(det), out, cls[by_image], nc, single))
    ev = coco_accumulate(recs, nc)
    return ev, coco_summarize(ev)


@pytest.mark.parametrize("name", list(U.SCENES))
def test_kernel_equals_restatement(name):
    batches, nc, single, arrays, imgs, ev, stats = U.reference(name)
    outs = [gpu_arrays(b, nc, single) for b in batches]
    for got, want in zip(outs, arrays):
        assert_arrays(got, want)
    pev, pstats = product_stats(batches, outs, nc, single)
    print(name, "stats", np.round(pstats, 6))
    assert np.abs(pstats - stats).max() <= TOL
    for key in ("precision", "recall", "scores"):
        assert pev[key].shape == ev[key].shape and np.abs(pev[key] - ev[key]).max() <= TOL, key


def test_no_labels_at_all():
    batch = U.scene(3, 300, 3, seed=5, no_label_imgs=(0, 1, 2))
    assert len(batch[3]) == 0 and batch[1].sum() > 0
    want, imgs = U.evaluate_batch(*batch, 3)
    got = gpu_arrays(batch, 3, False)
    assert_arrays(got, want)
    assert got["gt_ignore"].shape == (0, 4) and (got["matched"] == 0).all() and (got["ignored"] != 0).any()
    _, pstats = product_stats([batch], [got], 3, False)
    assert (pstats == -1).all()


def test_repeat_and_graph_capture_identical_bytes():
    from ydbl.engine.validator import coco_batch, group_labels

    batches, nc, single, arrays, *_ = U.reference("3x300x3")
    det, cnt, boxes, cls, bidx = batches[0]
    dev = torch.device("cuda")
    det_d, cnt_d = torch.from_numpy(det).to(dev), torch.from_numpy(cnt).to(dev)
    grouped = group_labels(boxes, cls, bidx, det.shape[0], dev)

    def call():
        return coco_batch(det_d, cnt_d, boxes, cls, bidx, nc, single, grouped=grouped)

    first, second = call(), call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = call()
    for k in KEYS:
        captured[k].fill_(7)
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        a = first[k].cpu().numpy().tobytes()
        assert a == second[k].cpu().numpy().tobytes() == captured[k].cpu().numpy().tobytes(), k
        assert np.array_equal(first[k].cpu().numpy(), arrays[0][k]), k
