"""The YOLOv10 baseline (yolov10n.yaml: SCDown, PSA, C2fCIB, v10Detect) on the host: construction from
tests/golden/yolov10.json, reference parameter names and shapes, the parser rules, the YAML route, RepVGGDW's fold,
shapes and routing from a meta-device plan, the scope guards, the new descriptor's layout -- and the yardstick
(tests/yolov10_util.py): the literal two-topk postprocess against the pinned-order sort.  No GPU."""

import copy
import ctypes as C
import json
import warnings

import pytest
import torch

import yolov10_util as U


@pytest.fixture(scope="module")
def pair():
    """(product YOLO, the unfused restatement) with the same weights; built once, left unchanged."""
    from ydbl import YOLO

    o = U.build_oracle("n", 3)
    p = YOLO(str(U.GOLDEN / "yolov10n.json"), nc=3)
    p.model.load_state_dict(o.state_dict(), strict=True)
    return p, o


def test_constructs_with_reference_names_and_shapes(pair):
    from ydbl.nn import modules as M

    p, o = pair
    sp, so = p.model.state_dict(), o.state_dict()
    assert list(sp) == list(so)  # no missing, no unexpected key, the reference's order
    assert all(sp[k].shape == so[k].shape for k in so)
    assert p.model.stride.tolist() == [8.0, 16.0, 32.0] and p.model.end2end is True
    layers = p.model.model
    assert isinstance(layers[5], M.SCDown) and isinstance(layers[7], M.SCDown) and isinstance(layers[20], M.SCDown)
    assert layers[5].cv2.conv.groups == layers[5].cv2.conv.out_channels == 128 and layers[5].cv2.conv.stride == (2, 2)
    assert isinstance(layers[5].cv2.act, torch.nn.Identity)
    psa = layers[10]
    assert isinstance(psa, M.PSA) and psa.c == 128
    assert (psa.attn.num_heads, psa.attn.head_dim, psa.attn.key_dim) == (2, 64, 32)
    cib = layers[22]
    assert isinstance(cib, M.C2fCIB) and len(cib.m) == 1 and isinstance(cib.m[0], M.CIB)  # 3 repeats x depth 0.33
    assert isinstance(cib.m[0].cv1[2], M.RepVGGDW) and cib.m[0].add is True
    head = layers[-1]
    assert isinstance(head, M.v10Detect) and head.end2end and head.max_det == 300 and head.legacy is False
    for seq in (*head.cv3, *head.one2one_cv3):
        assert type(seq[0][0]) is M.Conv and seq[0][0].conv.groups == seq[0][0].conv.in_channels
    assert all(a is not b for a, b in zip(head.cv2, head.one2one_cv2))
    want = torch.log(5 / 3 / (640 / head.stride) ** 2)
    from ydbl import YOLO

    fresh = YOLO(str(U.GOLDEN / "yolov10n.json"), nc=3).model.model[-1]  # bias_init covers both sets
    for branches in (fresh.cv3, fresh.one2one_cv3):
        torch.testing.assert_close(torch.stack([b[-1].bias.data[0] for b in branches]), want)
    for branches in (fresh.cv2, fresh.one2one_cv2):
        assert all(bool((b[-1].bias.data == 1.0).all()) for b in branches)


def test_parser_rules():
    """SCDown, PSA and C2fCIB take (c1, c2) with width scaling, C2fCIB the repeat count as an argument
    (U/nn/tasks.py:985-1075); v10Detect gets the channel list like Detect."""
    from ydbl.nn import modules as M
    from ydbl.nn.tasks import parse_model

    d = {"nc": 3, "scales": {"n": [0.33, 0.25, 1024], "l": [1.0, 1.0, 512]}, "scale": "n",
         "backbone": [[-1, 1, "Conv", [64, 3, 2]], [-1, 1, "SCDown", [1024, 3, 2]], [-1, 1, "PSA", [1024]],
                      [-1, 3, "C2fCIB", [1024, True, True]], [-1, 3, "C2fCIB", [512, True]]],
         "head": [[[2, 3, 4], 1, "v10Detect", ["nc"]]]}
    model, _ = parse_model(json.loads(json.dumps(d)))
    assert type(model[1]) is M.SCDown and model[1].cv1.conv.out_channels == 256
    assert type(model[2]) is M.PSA and model[2].c == 128 and model[2].cv2.conv.out_channels == 256
    assert type(model[3]) is M.C2fCIB and len(model[3].m) == 1 and type(model[3].m[0].cv1[2]) is M.RepVGGDW
    assert type(model[4]) is M.C2fCIB and type(model[4].m[0].cv1[2]) is M.Conv  # lk=False
    assert type(model[5]) is M.v10Detect and model[5].nl == 3 and model[5].nc == 3
    d["scale"] = "l"
    model, _ = parse_model(json.loads(json.dumps(d)))
    assert len(model[3].m) == 3 and model[3].cv2.conv.out_channels == 512  # min(1024, 512) x 1.0


def test_yaml_file_is_read_itself(tmp_path, golden_dir):
    """The reference ships one file per scale (yolov10n.yaml with its own `scales`): an existing path is read as it
    is, at the scale of its name."""
    import yaml

    from ydbl import YOLO

    d = json.loads((golden_dir / "yolov10.json").read_text())
    (tmp_path / "yolov10n.yaml").write_text(yaml.safe_dump(d, default_flow_style=None).replace("null", "None"))
    a = YOLO(str(tmp_path / "yolov10n.yaml"), nc=3)
    b = YOLO(str(golden_dir / "yolov10n.json"), nc=3)
    assert [(k, tuple(v.shape)) for k, v in a.model.state_dict().items()] == [
        (k, tuple(v.shape)) for k, v in b.model.state_dict().items()]


def test_fuse_folds_repvggdw_like_the_reference(pair):
    """DetectionModel.fuse() leaves every RepVGGDW one 7x7 nn.Conv2d whose weights equal the restatement's fuse()
    (block.py:791-815) exactly (compared in fp64); the plan-time fold of the two-branch form gives the same weights;
    the fused form reloads its own state_dict and compiles to the same single launch."""
    from ydbl.nn import modules as M

    p, o = pair
    pm, om_ = copy.deepcopy(p.model), copy.deepcopy(o)
    reps = [m for m in pm.modules() if isinstance(m, M.RepVGGDW)]
    assert len(reps) == 1
    before = [m.folded() for m in reps]
    assert pm.fuse() is pm and pm.is_fused()
    U.fuse_model(om_)
    refs = [m for m in om_.modules() if isinstance(m, U.RepVGGDW)]
    for m, r, (w0, b0) in zip(reps, refs, before):
        assert isinstance(m.conv, torch.nn.Conv2d) and not hasattr(m, "conv1") and m.conv.kernel_size == (7, 7)
        assert torch.equal(m.conv.weight.double(), r.conv.weight.double())
        assert torch.equal(m.conv.bias.double(), r.conv.bias.double())
        w1, b1 = m.folded()
        assert torch.equal(w0, w1) and torch.equal(b0, b1)
    pm.load_state_dict(copy.deepcopy(pm.state_dict()), strict=True)
    for model in (p.model, pm):
        whats = [st.what for st in model.compile(1, 64, 64, torch.float16, device="meta").plan.steps]
        assert whats.count("RepVGGDW.dw7") + whats.count("CIB.dw+pw.k7s1") == 1


def test_meta_plan_shapes_and_routing(pair):
    """Shapes and strides out of the meta-device plan; a session-side plan holds one branch set only (three box and
    three class tails), one PSA.attn, one 7x7 depthwise launch, no torch step and no copy; the module-level forward
    plan holds both sets, the end2end decode and the top-k."""
    p, _ = pair
    cm = p.model.compile(2, 96, 160, torch.float16, device="meta")
    assert [(lv.n, lv.h, lv.w, lv.c) for lv in cm.levels] == [(2, 12, 20, 67), (2, 6, 10, 67), (2, 3, 5, 67)]
    whats = [st.what for st in cm.plan.steps]
    assert whats.count("PSA.attn") == 1 and whats.count("SPPF.pool5x3") == 1
    assert whats.count("RepVGGDW.dw7") == 1
    assert not any(w.startswith("torch.") or w == "copy" for w in whats)
    tails = [w for w in whats if w.startswith("DWConv+Conv1x1+1x1")]
    assert len(tails) == 3  # the one2one class tails; the one2many branches are not emitted
    both = [st.what for st in p.model.compile(2, 96, 160, torch.float16, device="meta", head_forward=True).plan.steps]
    assert sum(w.startswith("DWConv+Conv1x1+1x1") for w in both) == 6
    head0 = min(i for i, w in enumerate(whats) if w.startswith("Detect.box"))  # the head's first launch
    assert both[-2:] == ["Detect.decode e2e", "TopK"] and len(both) == len(whats) + (len(whats) - head0) + 2


def test_dbl_plan_is_unchanged(golden_dir):
    """A DBL-n plan holds exactly the launches the committed plan dump lists (tests/golden/session_plans_meta.json is
    checked by tests/test_session_plan_host.py; here: no launch of this pull request's entry points)."""
    from ydbl import YOLO

    cm = YOLO("yolov13n_DBL.yaml", nc=3).model.compile(2, 128, 128, torch.float16, device="meta")
    names = {st.fn.__name__ for st in cm.plan.steps}
    assert not names & {"ydbl_detect_topk", "ydbl_detect_decode_e2e"}
    assert not any(st.what.startswith(("CIB", "RepVGGDW", "TopK")) for st in cm.plan.steps)


def test_guards_raise_before_device_work(pair):
    from ydbl.engine.session import DetectSession

    p, _ = pair
    x = torch.rand(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="YOLOv10"):
        DetectSession(p.model, 1, 64, 64, torch.float16, fp8=True)
    with pytest.raises(NotImplementedError, match="YOLOv10"):
        p.session(1, 64, 64, fp8=True)
    with pytest.raises(NotImplementedError, match="E2EDetectLoss"):
        DetectSession(p.model, 1, 64, 64, torch.float16, loss={"max_labels": 8})
    with pytest.raises(NotImplementedError, match="E2EDetectLoss"):
        p.session(1, 64, 64, loss=True)
    with pytest.raises(NotImplementedError, match="E2EDetectLoss"):
        p.model.loss({"img": x, "batch_idx": torch.zeros(0), "cls": torch.zeros(0), "bboxes": torch.zeros(0, 4)})
    with pytest.raises(NotImplementedError, match="E2EDetectLoss"):
        p.model({"img": x})
    with pytest.raises(NotImplementedError, match="E2EDetectLoss"):
        p.val([{"img": x}], loss=True)


def test_attention_guard_holds_for_psa():
    """PSA reuses Attention.emit with its head_dim 64 / key_dim 32 guard: c1 = 128 gives num_heads = 1, head_dim 64
    (fine); a hand-made Attention of another shape inside it is refused at emit."""
    from ydbl.nn import modules as M
    from ydbl.runtime import Plan

    plan = Plan(torch.device("meta"), torch.float16)
    m = M.PSA(128, 128)
    assert (m.attn.num_heads, m.attn.head_dim, m.attn.key_dim) == (1, 64, 32)
    m.emit(plan, plan.alloc(1, 4, 4, 128))
    assert [st.what for st in plan.steps].count("PSA.attn") == 1
    m.attn = M.Attention(64, 2, 0.5)
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        m.emit(Plan(torch.device("meta"), torch.float16), plan.alloc(1, 4, 4, 128))


def test_augment_warns_once_and_builds_the_plain_session(pair, monkeypatch):
    from ydbl.engine import model as EM
    from ydbl.nn import tasks as T

    p, _ = pair
    monkeypatch.setattr(T, "_E2E_AUGMENT_WARNED", False)
    built = []
    monkeypatch.setattr(EM.Model, "_cached_session", lambda self, key, dev, build: built.append(key) or key)
    monkeypatch.setattr(EM, "select_device", lambda d=None: torch.device("cpu"))
    with pytest.warns(UserWarning, match="End2End"):
        k1 = p.session(2, 64, 64, augment=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        k2 = p.session(2, 64, 64, augment=True)  # once
        k3 = p.session(2, 64, 64)
    assert k1 == k2 == k3  # the plain session's key: nothing augmented is built


def test_topk_desc_layout_matches_c(tmp_path):
    from test_yolo11_host import _layout
    from ydbl import _lib

    _layout(tmp_path, "ydbl_topk_desc", _lib.TopkDesc)


def test_nms_takes_the_six_column_branch():
    """ydbl.utils.ops.non_max_suppression on a [B, N, 6] prediction: the reference's lines 224-228."""
    from ydbl.utils.ops import non_max_suppression

    g = torch.Generator().manual_seed(3)
    pred = torch.rand(2, 40, 6, generator=g)
    pred[..., 4] = pred[..., 4].sort(dim=1, descending=True).values
    pred[..., 5] = torch.randint(0, 4, (2, 40), generator=g).float()
    for classes in (None, [1, 3]):
        got = non_max_suppression(pred, conf_thres=0.3, max_det=9, classes=classes)
        for b in range(2):
            assert torch.equal(got[b], U.reference_tail(pred[b], 0.3, 9, classes))
    assert len(got[0]) < 9


# ----------------------------------------------------------------------------------------------- the yardstick
def _distinct_scores(A, nc, seed):
    """[A, nc] scores from a permutation of a strictly increasing grid in (0, 1): distinct by construction."""
    g = torch.Generator().manual_seed(seed)
    grid = (torch.arange(A * nc, dtype=torch.float32) + 1) / (A * nc + 1)
    assert bool((grid[1:] > grid[:-1]).all())
    return grid[torch.randperm(A * nc, generator=g)].view(A, nc)


@pytest.mark.parametrize("A,nc,max_det", [(21, 3, 300), (84, 3, 300), (84, 1, 7), (400, 80, 300), (1000, 5, 300),
                                          (300, 2, 300), (301, 2, 300), (50, 7, 1)])
def test_two_topks_equal_the_pinned_sort_on_distinct_scores(A, nc, max_det):
    """Detect.postprocess (head.py:200-221), word for word, equals the k largest of all (anchor, class) scores in
    (score desc, anchor * nc + class asc) order when the scores are distinct: a pair of an anchor outside the first
    top-k has k pairs at least as large ahead of it."""
    for seed in range(3):
        sc = _distinct_scores(A, nc, 100 * A + seed)
        bx = torch.rand(A, 4, generator=torch.Generator().manual_seed(seed)) * 100
        lit = U.postprocess(torch.cat([bx, sc], 1)[None], max_det, nc)[0]
        pin = U.select_pinned(bx, sc, k_head=min(max_det, A), conf=-1.0, max_det=max_det)
        assert lit.shape == (min(max_det, A), 6)
        assert torch.equal(lit, pin)
        # and the six-column tail of the NMS on top of it
        for conf, md, classes in ((0.5, 300, None), (0.2, 5, [0]), (0.0, 300, [nc - 1])):
            want = U.reference_tail(lit, conf, md, classes)
            got = U.select_pinned(bx, sc, k_head=min(max_det, A), conf=conf, max_det=md, classes=classes)
            assert torch.equal(want, got)


def test_select_candidates_ignores_list_order():
    g = torch.Generator().manual_seed(5)
    n = 500
    box, sc = torch.rand(n, 4, generator=g), (torch.randint(1, 50, (n,), generator=g).float() / 64)  # many ties
    idx = torch.randperm(4000, generator=g)[:n].int()
    a = U.select_candidates(box, sc, (idx % 3).int(), idx, 100)
    perm = torch.randperm(n, generator=g)
    b = U.select_candidates(box[perm], sc[perm], (idx[perm] % 3).int(), idx[perm], 100)
    assert torch.equal(a, b) and len(a) == 100
    assert bool((a[1:, 4] <= a[:-1, 4]).all())
