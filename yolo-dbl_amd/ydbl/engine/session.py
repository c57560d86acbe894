"""One compiled inference configuration: forward + Detect decode + NMS as a single launch plan.

The plan is captured into a hipGraph on first use and replayed afterwards, so
a batch costs one H2D/D2D copy into the static input buffer plus one graph
launch.  Outputs are fixed-shape device buffers ``det [B, max_det, 6]``
(x1, y1, x2, y2, conf, cls) and ``count [B]`` — the all-gather friendly
layout used by the multi-GPU path.

BatchSession is what the three session kinds share: a batch, possibly split into sub-batch plans, loaded through
the staging buffers and replayed as one graph.  DetectOptions is the one record of a detection session's settings.
"""

from __future__ import annotations

import operator
import warnings
import weakref
from dataclasses import dataclass

import torch

from .. import _lib
from .._lib import DecodeAug, DecodeDesc, ScaleImgDesc
from ..runtime import BranchGraphRunner, GraphRunner, Plan
from ..tail import E2ETail, NmsTail


SPLIT_MIN_BATCH = 4  # the benched layouts: DBL-n bs32 / DBL-s bs8, bs64 / DBL-l 1280 bs8 (bench.py --streams 2)


def default_streams(batch: int) -> int:
    """Sub-batch graphs of the session predict() / DetectionModel.forward build for a batch: 2 from batch 4 up -- the
    layout bench.py times (DBL-n bs32 +3 %, DBL-s bs64 +9 %, DBL-l 1280 bs8 +8.5 % over one graph;
    3-4 branches measured slower) -- else 1 (a bs1 branch per image leaves most of the chip idle)."""
    return 2 if batch >= SPLIT_MIN_BATCH else 1


@dataclass(frozen=True)
class DetectOptions:
    """Every setting of a detection session (DetectSession, AugmentSession) besides its shape and placement, in the
    order the constructors take them positionally.  Built once by the public constructor and handed as it is to the
    sub-batch sessions; Model.session() derives its cache key from the fields, so a new field is in the key by
    construction.  fp8 = True: every candidate conv in e4m3, a float in (0, 1): that share of the candidates' MACs,
    least output-sensitive first (ydbl.quant.enable_fp8); fp8_calibration: an Fp8Calibration / its file, applied at
    the first launch; loss = {"max_labels", "topk", "gains"[, "debug"]}: ydbl_detect_loss behind the head."""

    dtype: torch.dtype = torch.float16
    conf: float = 0.25
    iou: float = 0.7
    max_det: int = 300
    multi_label: bool = False
    agnostic: bool = False
    classes: tuple | None = None
    max_nms: int = 30000
    max_wh: float = 7680
    clip: bool = True
    keep_pred: bool = False
    use_graph: bool = True
    nms: bool = True
    fp8: bool | float = False
    fp8_calibration: object = None
    loss: dict | None = None

    def __post_init__(self):
        if self.classes is not None and type(self.classes) is not tuple:
            object.__setattr__(self, "classes", tuple(self.classes))


def _options(options, args, kw) -> DetectOptions:
    if options is None:
        return DetectOptions(*args, **kw)
    if args or kw:
        raise TypeError("options= takes the place of the single settings")
    return options


class BoundOutputs:
    """A predict() call's outputs in a session's binding slot (DetectSession.launch_bound): det [B, max_det, 6],
    count [B] and LoadTensor's scale, valid as views of the slot until detach() copies them out (on first access, or
    when the slot comes round again while this object is alive)."""

    def __init__(self, det, count, flat, scale, event=None):
        self.det, self.count, self.flat, self.scale, self.own = det, count, flat, scale, False
        self.event = event  # recorded after the replay that wrote the slot

    def detach(self):
        if not self.own:
            if self.event is not None:  # the copy may be issued from another stream than the replay's
                torch.cuda.current_stream(self.flat.device).wait_event(self.event)
            flat = self.flat.clone()
            n = self.det.numel()
            self.det, self.count = flat[:n].view(self.det.shape), flat[n:].view(torch.int32)
            self.flat, self.scale, self.own = flat, self.scale.clone(), True
        return self


class _EagerSlot:
    """use_graph=False: a binding slot's launches run eagerly (the descriptors are pointed at the slot per run)."""

    def __init__(self, session, k, pre):
        self.s, self.k, self.pre = session, k, pre

    def replay(self):
        det, count, _, _ = self.s._pout[self.k]
        self.s._set_slot(self.k, det, count)
        self.pre.run()
        for p in self.s.plans:
            p.run()
        self.s._set_slot(0)


def is_segment(model) -> bool:
    """The model's head is a Segment (U/nn/modules/head.py:224-271): its sessions also produce masks."""
    from ..nn.modules import Segment

    return isinstance(model.model[-1], Segment)


def check_segment(model, fp8=False, loss=None, gather_rows=None):
    """A segmentation model's scope guards, on the host before any device work: no fp8 (no calibration record covers
    Proto and the coefficient branch), no loss (the criterion is v8SegmentationLoss, U/utils/loss.py) and no
    batch-sharded predictor (its record rows carry boxes only)."""
    if not is_segment(model):
        return
    if fp8:
        raise NotImplementedError("fp8=True on a segmentation model: no calibration record exists for Proto and the "
                                  "mask-coefficient branch")
    if loss is not None and loss is not False:
        raise NotImplementedError("the loss of a segmentation model is v8SegmentationLoss, which is not implemented")
    if gather_rows is not None:
        raise NotImplementedError("segmentation models are not implemented for the batch-sharded predictor "
                                  "(gather_rows): its record rows carry boxes only")


def is_pose(model) -> bool:
    """The model's head is a Pose (U/nn/modules/head.py:328-401): its sessions also produce keypoints."""
    from ..nn.modules import Pose

    return isinstance(model.model[-1], Pose)


def check_pose(model, fp8=False, loss=None, gather_rows=None):
    """A pose model's scope guards, on the host before any device work: no fp8 (no calibration record covers the
    keypoint branch), no loss (the criterion is v8PoseLoss, U/utils/loss.py) and no batch-sharded predictor (its
    record rows carry boxes only)."""
    if not is_pose(model):
        return
    if fp8:
        raise NotImplementedError("fp8=True on a pose model: no calibration record exists for the keypoint branch")
    if loss is not None and loss is not False:
        raise NotImplementedError("the loss of a pose model is v8PoseLoss, which is not implemented")
    if gather_rows is not None:
        raise NotImplementedError("pose models are not implemented for the batch-sharded predictor "
                                  "(gather_rows): its record rows carry boxes only")


def _f32(v: float) -> float:
    """v rounded to fp32, as torch does when it multiplies a Python float into an fp32 tensor."""
    return torch.tensor(v, dtype=torch.float32).item()


def _of_tail(path: str, join=None) -> property:
    """A read-only session attribute that lives on the session's tail (ydbl.tail); join: what a split session makes
    of its sub-batch sessions' values (else it has none)."""
    get = operator.attrgetter(path)

    def read(self):
        return join([read(c) for c in self.children]) if join and self.children else get(self.tail)

    return property(read)


def _det_count(batch: int, max_det: int, dev):
    """det [B, max_det, 6] fp32 and count [B] int32 as views of ONE zeroed buffer (flat), so a caller keeping a batch's
    outputs past the next launch copies them in one go (predict())."""
    flat = torch.zeros(batch * max_det * 6 + batch, dtype=torch.float32, device=dev)
    return flat[: batch * max_det * 6].view(batch, max_det, 6), flat[batch * max_det * 6:].view(torch.int32), flat


class BatchSession:
    """A batch, possibly split, replayed as one graph: what DetectSession, AugmentSession and EmbedSession share.

    streams = k > 1 (and batch >= k): the batch is split into k contiguous sub-batches (parallel.shard_bounds) --
    ``bounds``, [(0, batch)] when unsplit -- each a session of the same kind in ``children`` (empty when unsplit) with
    its own launch plan and buffers, writing its rows of the parent's shared outputs.  ``plans`` holds the plans in
    row order, ``plan`` the first.  launch() replays them as ONE hipGraph -- a GraphRunner, or the k plans as the
    branches of a BranchGraphRunner -- or, with use_graph=False, runs them eagerly, a split session's on one side
    stream per plan (made on the first such launch) with a fork / join around them.

    A subclass sets up its outputs, then calls _build(): that asks _child(i, a, b) for the session of rows a:b (built
    onto slices of the outputs) when split, else _compile() for the session's own plan (which sets ``compiled``)."""

    _bound = None
    fp8 = fp8_ready = False  # only a DetectSession has e4m3 operands, calibrated at its first launch

    def __init__(self, model, batch: int, h: int, w: int, dtype, use_graph, device, streams):
        from ..parallel import shard_bounds

        self.model, self.batch, self.h, self.w, self.dtype = model, batch, h, w, dtype
        self.use_graph, self.device = use_graph, torch.device(device)
        split = streams > 1 and batch >= streams
        self.bounds = [shard_bounds(batch, streams, r) for r in range(streams)] if split else [(0, batch)]
        self.children, self._graph, self._side = [], None, None

    def _build(self):
        if len(self.bounds) > 1:
            self.children = [self._child(i, a, b) for i, (a, b) in enumerate(self.bounds)]
            self.plans = [c.plan for c in self.children]
        else:
            self.plans = [self._compile()]
        self.plan = self.plans[0]

    @property
    def parts(self):
        """The sessions that own a plan, in row order: the children, or the unsplit session itself."""
        return self.children or [self]

    def load(self, x: torch.Tensor, scale: torch.Tensor | None = None):
        """Copy a BCHW batch into the static input buffer(s) (LoadTensor semantics are the caller's); scale: a 0-dim
        fp32 device tensor the batch is multiplied by on the way in (x * fp32(1/255) is what torch's GPU division by
        255.0 computes, so no host sync is needed for it)."""
        self._bound = None
        parts = self.parts
        shape = (self.batch, *parts[0].compiled.input.shape[1:])
        if tuple(x.shape) != shape:
            raise ValueError(f"input shape {tuple(x.shape)} != session shape {shape}")
        for p, (a, b) in zip(parts, self.bounds):
            xs = x[a:b] if self.children else x
            if scale is None:
                p.compiled.input.copy_(xs, non_blocking=True)
            else:  # fp32 before the scale: x.float() / 255.0 as LoadTensor computes it (U/data/loaders.py:566)
                torch.mul(xs if xs.dtype == torch.float32 else xs.float(), scale, out=p.compiled.input)

    def launch(self):
        if self.fp8 and not self.fp8_ready:  # (DetectSession) a given calibration, else the first batch calibrates
            self.calibrate_fp8(calibration=self.fp8_calibration)  # (dynamic post-training quantization)
        if self.use_graph:
            g = self._graph
            if g is None:  # every sub-batch plan a branch of one graph: one launch
                g = self._graph = BranchGraphRunner(self.plans) if self.children else GraphRunner(self.plan)
            g.replay()
        elif self.children:  # eager: each sub-batch plan on its own stream, then join
            dev = self.plan.buffers[0].device
            if self._side is None:
                self._side = [torch.cuda.Stream(dev) for _ in self.plans]
            cur = torch.cuda.current_stream(dev)
            for p, st in zip(self.plans, self._side):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    p.run()
            for st in self._side:
                cur.wait_stream(st)
        else:
            self.plan.run()

    def __call__(self, x: torch.Tensor | None = None, scale: torch.Tensor | None = None):
        if x is not None:
            self.load(x, scale)
        self.launch()
        return self.outputs()


class DetectSession(BatchSession):
    """``DetectSession(model, batch, h, w, dtype, conf=..., ..., device=, streams=, gather_rows=)``: the settings, in
    DetectOptions' order and under its names, or ``options=`` a ready record.

    streams = k > 1: the batch is split into k contiguous sub-batches, each compiled into its own launch
    plan (own buffers) writing into slices of the shared det / count (/ pred) outputs; the k plans are captured
    as k independent branches of ONE hipGraph (BatchSession; eager mode: one HIP stream per plan).
    At DBL-n/s sizes every launch is short and ramp/tail-bound, so two concurrent half-batch branches fill each
    other's gaps (scripts/stream_probe.py: DBL-n bs32 +10 %, DBL-s bs64 +14 %; one two-branch graph instead of
    two graphs on two streams a further +2.5 %, scripts/graph_branch_probe.py).

    ``tail`` is the detection tail behind the forward (ydbl.tail: an NmsTail, or an E2ETail behind an end2end head),
    built by _compile(); a split session's children have one each.
    sparse_box: the session runs the sparse box path (NmsTail.sparse_box) -- its P3 / P4 box logits exist
    only in the 8 x 16 tiles that hold an NMS candidate of the last batch (see feats())."""

    end2end = False
    records = loss = out_flat = tail = None

    def __init__(self, model, batch: int, h: int, w: int, *args, device="cuda", streams=1, gather_rows=None,
                 options=None, _outputs=None, _bind=None, **kw):
        opt = _options(options, args, kw)
        if opt.fp8 and opt.dtype != torch.float16:
            raise ValueError("fp8 operands run on the fp16 activation path (half=True)")
        if opt.fp8 and any(type(m).__name__ == "A2C2f" for m in model.modules()):
            raise NotImplementedError("fp8=True on a model with A2C2f: no calibration record exists for the "
                                      "area-attention blocks")
        # an end2end head (v10Detect): the tail is a top-k, not an NMS (tail.E2ETail)
        self.end2end = bool(getattr(model.model[-1], "end2end", False))
        if self.end2end and opt.fp8:
            raise NotImplementedError("fp8=True on an end2end (YOLOv10) model: no calibration record exists for the "
                                      "YOLOv10 baseline")
        if self.end2end and opt.loss is not None:
            from ..nn.tasks import check_e2e_loss

            check_e2e_loss(model)
        check_segment(model, opt.fp8, opt.loss, gather_rows)  # a Segment head: no fp8, loss or record rows
        check_pose(model, opt.fp8, opt.loss, gather_rows)  # a Pose head: the same three
        if opt.fp8:
            for name in ("C2PSA", "SPPF"):
                if any(type(m).__name__ == name for m in model.modules()):
                    raise NotImplementedError(f"fp8=True on a model with {name}: no calibration record exists for "
                                              "the YOLO11 / YOLOv8 baselines")
        # loss: ydbl_detect_loss behind the head (_emit_loss).  The loss normalises by the whole batch's target scores,
        # so the batch stays one plan, and it reads every level's box logits, so the levels stay dense (no sparse box
        # path)
        if opt.loss is not None:
            if gather_rows is not None:
                raise NotImplementedError("loss is not implemented for the batch-sharded predictor (gather_rows)")
            streams = 1
        self._init_detect(model, batch, h, w, opt, device, streams)
        fp8 = opt.fp8
        self.fp8_fraction = float(fp8) if not isinstance(fp8, bool) and 0 < float(fp8) < 1 else 1.0
        # predict()'s in-place path (launch_bound): binding slot 0 is the session's own staging buffer (load()), slots
        # 1 and 2 alternate between predict() calls, each with its own graph (LoadTensor maximum + the plans) and its
        # own det | count outputs, kept until the slot comes round again (then copied if its Results still live)
        self._calls, self._slot_ptrs, self._pgraph, self._pout, self._pheld = 0, {}, {}, {}, {}
        self._max_work = {}  # per binding slot: the batch-max kernel's tickets are reset by its last block
        # the last launch_bound() replay (the slots share the plans' activation buffers): its stream and, per slot, an
        # event recorded after it -- a call from another stream waits for it, detach() waits for its slot's
        self._last_stream, self._slot_ev = None, {}
        A = sum((h // int(st)) * (w // int(st)) for st in model.model[-1].stride.tolist())
        if _outputs is None and gather_rows is not None:
            # one record per image [det (max_det*6 fp32) | count (int32) | pad]: the boxes and counts of a batch-
            # sharded predict leave the GPU in ONE all-gather (ydbl.parallel); rows >= batch stay empty padding
            from ..parallel import record_views, record_width

            if gather_rows < batch:
                raise ValueError(f"gather_rows {gather_rows} < batch {batch}")
            self.records = torch.zeros((gather_rows, record_width(self.max_det)), dtype=torch.float32,
                                       device=self.device)
            det_v, cnt_v = record_views(self.records[:batch], self.max_det)
            _outputs = (det_v, cnt_v, torch.empty((batch, 4 + self.nc, A), dtype=torch.float32, device=device)
                        if opt.keep_pred else None)
        if _outputs is not None:  # record rows, or slices of a split session's shared outputs
            self.det, self.count, self.pred, *kp = _outputs
            self.kpts = kp[0] if kp else None
        elif len(self.bounds) > 1:
            self._alloc_outputs(A)
        self._bind = _bind
        if _bind is None:  # a top-level session owns the binding slots (a split session's children get views): per
            # slot one batch-pointer word per sub-batch plan and one batch maximum for all (launch_bound())
            self.bind_ptrs = torch.empty((3, len(self.bounds)), dtype=torch.int64, device=self.device)
            self.bind_amax = torch.zeros((3, 1), dtype=torch.float32, device=self.device)
        self._build()
        if self.children:
            self.A = self.children[0].A
        if _bind is None:
            own = torch.tensor([p.compiled.input.data_ptr() for p in self.parts], dtype=torch.int64)
            self.bind_ptrs.copy_(own.expand(3, -1))

    def _init_detect(self, model, batch, h, w, opt: DetectOptions, device, streams):
        """What every detection session has, binding or not: the record and the attributes read from outside."""
        BatchSession.__init__(self, model, batch, h, w, opt.dtype, opt.use_graph, device, streams)
        self.opt = opt
        self.fp8, self.fp8_ready, self.fp8_calibration = bool(opt.fp8), False, opt.fp8_calibration
        self.conf, self.iou, self.max_det = float(opt.conf), float(opt.iou), int(opt.max_det)
        self.nc = model.model[-1].nc
        self.det = self.count = self.pred = None
        self.segment = is_segment(model)  # a Segment head: the NMS also writes keep_idx, masks() reads plan.seg
        self.pose = is_pose(model)  # a Pose head: keep_idx too, and ydbl_pose_keypoints behind the NMS writes kpts
        self.kpts = None

    def _alloc_outputs(self, A: int):
        self.det, self.count, self.out_flat = _det_count(self.batch, self.max_det, self.device)
        self.pred = (torch.empty((self.batch, 4 + self.nc, A), dtype=torch.float32, device=self.device)
                     if self.opt.keep_pred else None)
        if self.pose and self.opt.nms:  # [B, max_det, K, ndim]: one buffer, each sub-batch plan writes its rows
            K, ndim = self.model.model[-1].kpt_shape
            self.kpts = torch.zeros((self.batch, self.max_det, K, ndim), dtype=torch.float32, device=self.device)

    def _child(self, i: int, a: int, b: int):
        outs = (self.det[a:b], self.count[a:b], self.pred[a:b] if self.pred is not None else None,
                self.kpts[a:b] if self.kpts is not None else None)
        return DetectSession(self.model, b - a, self.h, self.w, device=self.device, options=self.opt, _outputs=outs,
                             _bind=(self.bind_ptrs[0, i:i + 1], self.bind_amax[0]))

    def _compile(self) -> Plan:
        opt = self.opt
        bind = self._bind or (self.bind_ptrs[0], self.bind_amax[0])
        cm = self.compiled = self.model.compile(self.batch, self.h, self.w, self.dtype, device=self.device, bind=bind)
        plan = cm.plan
        self.A = sum(lv.h * lv.w for lv in cm.levels)
        if self.det is None:
            self._alloc_outputs(self.A)
        head, outs = self.model.model[-1], (self.det, self.count, self.pred)
        if self.end2end:  # (v10Detect) the tail is a top-k, not an NMS
            tail = self.tail = E2ETail(plan, self.batch, self.A, head, opt, *outs)
            tail.emit_decode(cm.levels)
            tail.emit_topk(self.h, self.w)
            return plan
        tail = self.tail = NmsTail(plan, self.batch, self.A, head, opt, *outs, segment=self.segment, pose=self.pose,
                                   kpts=self.kpts)
        dd = tail.emit_decode(cm.levels)
        tail.emit_nms(self.h, self.w)
        if self.pose:  # the kept rows' keypoints, inside the graph
            tail.emit_keypoints(plan.pose)
        if opt.loss is not None:
            self._emit_loss(plan, cm, dd, opt.loss)
        return plan

    def _emit_loss(self, plan: Plan, cm, dd: DecodeDesc, cfg: dict):
        """ydbl_detect_loss as the plan's last step, reading the level buffers in place: self.loss (utils.loss
        LossBuffers) holds gt [B, max_labels, 5] -- refilled by load_labels() before a replay, like the input -- and
        the outputs loss [3], target_scores_sum, per_image [B, 3]."""
        from ..utils.loss import MAX_LABELS, LossBuffers, loss_gains

        det, nl = cm.detect, len(cm.levels)
        self.loss = LossBuffers(list(dd.box)[:nl], list(dd.cls)[:nl], det.stride.tolist(), det.nc,
                                cfg.get("gains") or loss_gains(self.model), cfg.get("max_labels", MAX_LABELS),
                                cfg.get("topk", 10), plan.device, debug=bool(cfg.get("debug")), reg_max=det.reg_max)
        plan.buffers += self.loss.tensors()
        plan.launch("ydbl_detect_loss", self.loss.desc, what="Detect.loss", keep=[self.loss, dd])

    def load_labels(self, gt: torch.Tensor):
        """Refill the loss step's label buffer from a padded host / device tensor [B, max_labels, 5] (utils.loss
        pad_targets) before the next launch."""
        if self.loss is None:
            raise RuntimeError("load_labels(): the session was built without loss=")
        if tuple(gt.shape) != tuple(self.loss.gt.shape):
            raise ValueError(f"label buffer shape {tuple(gt.shape)} != {tuple(self.loss.gt.shape)}")
        self.loss.gt.copy_(gt, non_blocking=True)

    # ------------------------------------------------------------------ instance masks (a Segment head)
    def seg_outputs(self):
        """(mc [B, nm, A], p [B, nm, mh, mw]) of the last launch as fresh tensors of the session's dtype: the
        reference's Segment.forward outputs (U/nn/modules/head.py:259-271)."""
        from ..nn.modules import seg_coefficients

        if not self.segment:
            raise RuntimeError("seg_outputs(): the model's head is not a Segment")
        segs = [p.compiled.plan.seg for p in self.parts]
        return (torch.cat([seg_coefficients(mcs) for _, mcs in segs]),
                torch.cat([proto.nchw().contiguous() for proto, _ in segs]))

    def _mask_views(self, part, i=None):
        """The proto and coefficient views of one sub-batch plan (whole, or image i of it alone) as _lib.View."""
        proto, mcs = part.compiled.plan.seg
        if i is None:
            return proto.struct(), [v.struct() for v in mcs]

        def one(v):
            st = v.struct()
            st.ptr += i * v.h * v.w * v.cs * v.base.element_size()
            st.n = 1
            return st

        return one(proto), [one(v) for v in mcs]

    def _check_masks(self, what: str):
        if not self.segment or not self.opt.nms:
            raise RuntimeError(f"{what}(): needs a Segment head and a session with nms=True")

    def _masks(self, what: str, counts, width: int, dtype, out_dtype=None):
        """masks() / masks_bits(): the rows' offsets and one ydbl_process_mask launch per sub-batch plan into
        out [sum(counts), h, width] of `dtype` -> (out, offsets [B + 1])."""
        from ..utils.ops import launch_process_mask

        self._check_masks(what)
        offs = [0]
        for c in counts:
            offs.append(offs[-1] + int(c))
        out = torch.empty((offs[-1], self.h, width), dtype=dtype, device=self.device)
        if offs[-1] == 0:
            return out, offs
        row = torch.tensor(offs[:-1], dtype=torch.int64).to(self.device, non_blocking=True)
        for part, (a, b) in zip(self.parts, self.bounds):
            slots = max(counts[a:b])
            if slots == 0:
                continue
            pv, mcv = self._mask_views(part)
            launch_process_mask(pv, self.det[a:b], self.count[a:b], row[a:b], out, (self.h, self.w),
                                window=(0, 0, pv.h, pv.w), sx=_f32(pv.w / self.w), sy=_f32(pv.h / self.h),
                                crop_after=False, max_det=self.max_det, det_stride=self.det.stride(0),
                                keep_idx=part.keep_idx, mc=mcv, nc=self.nc if part.multi_label else 0, slots=slots,
                                out_dtype=out_dtype)
        return out, offs

    def masks(self, counts, dtype=torch.float32):
        """process_mask(upsample=True) of the last launch's detections (U/models/yolo/segment/predict.py:56-57): one
        ydbl_process_mask launch per sub-batch plan on the current stream, reading the plan's proto and coefficient
        buffers and the session's det / count / keep_idx in place -- call it before the session is launched again.
        counts: the host copy of self.count.  -> (masks [sum(counts), h, w] 0 / 1 in `dtype`, offsets [B + 1])."""
        return self._masks("masks", counts, self.w, dtype)

    def masks_bits(self, counts):
        """masks() as bit planes (YDBL_MASK_BITS, include/ydbl.h): the same 0 / 1 values, 64 columns to a word, 1/32
        of the fp32 bytes -- what ydbl_mask_iou reads.  One ydbl_process_mask launch per sub-batch plan on the current
        stream, under masks()' conditions.  -> (words int64 [sum(counts), h, ceil(w / 64)], offsets [B + 1]); bit j
        of word q of a row is column 64 q + j, bits past w are 0."""
        return self._masks("masks_bits", counts, (self.w + 63) // 64, torch.int64, _lib.MASK_BITS)

    def masks_native(self, i, boxes, shape, dtype=torch.float32):
        """process_mask_native of image i of the last launch (retina_masks, predict.py:53-55): boxes [k, >= 4] fp32 on
        the device, already scaled to `shape` = the original image's (h, w), row j the session's j-th kept detection
        of the image.  One launch on the current stream -> masks [k, shape[0], shape[1]] 0 / 1 in `dtype`."""
        from ..utils.ops import launch_process_mask, mask_window

        self._check_masks("masks_native")
        k = boxes.shape[0]
        out = torch.empty((k, int(shape[0]), int(shape[1])), dtype=dtype, device=self.device)
        if k == 0:
            return out
        part, a = next((p, a) for p, (a, b) in zip(self.parts, self.bounds) if a <= i < b)
        pv, mcv = self._mask_views(part, i - a)
        boxes = boxes.contiguous()
        zero = torch.zeros(1, dtype=torch.int64, device=self.device)
        launch_process_mask(pv, boxes, self.count[i:i + 1], zero, out, shape, window=mask_window(pv.h, pv.w, shape),
                            sx=1.0, sy=1.0, crop_after=True, max_det=self.max_det, det_row=boxes.shape[1],
                            keep_idx=part.keep_idx[i - a], mc=mcv, nc=self.nc if part.multi_label else 0, slots=k)
        return out

    # ------------------------------------------------------------------ keypoints (a Pose head)
    def pose_outputs(self):
        """kpt [B, nk, A] of the last launch as a fresh tensor of the session's dtype: the raw keypoint maps, the
        reference's Pose.forward output (U/nn/modules/head.py:367)."""
        from ..nn.modules import pose_raw

        if not self.pose:
            raise RuntimeError("pose_outputs(): the model's head is not a Pose")
        return torch.cat([pose_raw(p.compiled.plan.pose) for p in self.parts])

    # What the tail owns, under the names it has on a session; a split session has them on its children only, except:
    cand_box, cand_score, cand_cls, cand_idx = (_of_tail("cands." + n) for n in ("box", "score", "cls", "idx"))
    cap, multi_label, keep_idx, tile_masks = (_of_tail(n) for n in ("cap", "multi_label", "keep_idx", "tile_masks"))
    classes_t = _of_tail("classes")
    cand_count = _of_tail("cands.count", torch.cat)  # candidates per image of the last launch
    fused_candidates, sparse_box = _of_tail("fused", all), _of_tail("sparse", all)  # (true of every sub-batch plan)

    # ------------------------------------------------------------------ execution
    def can_bind(self, x: torch.Tensor) -> bool:
        """launch_bound() takes x: a contiguous fp32 tensor of the session's shape on its device, every sub-batch 16-byte
        aligned (the stem kernels' vector loads)."""
        if self.records is not None:  # gather_rows: the NMS writes record rows (out_stride = record width), not slots
            return False
        if self.segment:  # the masks are assembled from the session's own det / count / keep_idx after the replay
            return False
        if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.device != self.det.device
                or not x.is_contiguous() or tuple(x.shape) != (self.batch, 3, self.h, self.w)
                or (self.fp8 and not self.fp8_ready)):  # (an uncalibrated fp8 session calibrates on a loaded batch)
            return False
        per = 3 * self.h * self.w * 4
        return all((x.data_ptr() + a * per) % 16 == 0 for a, _ in self.bounds)

    def _set_slot(self, k: int, det: torch.Tensor | None = None, count: torch.Tensor | None = None):
        """Point the plans' input-reading launches at binding slot k and their NMS outputs at det / count (default:
        the session's own), before a capture; the C-ABI copies both into the kernel arguments at launch."""
        parts = self.parts
        for i, p in enumerate(parts):  # slot 0: no binding, the plans read their own staging buffers
            p.compiled.set_bind(self.bind_ptrs[k, i:i + 1] if k else None, self.bind_amax[k])
        det = self.det if det is None else det
        count = self.count if count is None else count
        nds = [st.args[0] for p in parts for st in p.plan.steps if st.fn.__name__ in ("ydbl_nms", "ydbl_detect_topk")]
        for nd, (a, b) in zip(nds, self.bounds):
            nd.out, nd.out_count = det[a:b].data_ptr(), count[a:b].data_ptr()
        # a Pose head: the keypoint launch reads the slot's counts; kpts stays the session's own buffer (the caller
        # copies it behind the replay: Model.predict)
        kds = [st.args[0] for p in parts for st in p.plan.steps if st.fn.__name__ == "ydbl_pose_keypoints"]
        for kd, (a, b) in zip(kds, self.bounds):
            kd.count = count[a:b].data_ptr()

    def launch_bound(self, x: torch.Tensor) -> "BoundOutputs":
        """predict()'s path for a device batch: the plans read x in place (include/ydbl.h ydbl_input_bind) -- no
        staging copy -- and apply LoadTensor's /255 rule (U/data/loaders.py:561-566) from x's maximum, which the
        launch computes on the device first (ydbl_batch_max_bound, the first node of the same graph: no host sync).
        Calls alternate between two binding slots, each with its own captured graph and its own det | count
        outputs, so nothing is copied per call: the outputs stay in the slot until it comes round again, and are
        copied then only if the call's BoundOutputs (its Results) are still alive -- or on first access."""
        if not self.can_bind(x):
            raise ValueError("launch_bound(): a contiguous fp32 batch of the session's shape on its device, 16-byte "
                             "aligned")
        k = 1 + self._calls % 2
        self._calls += 1
        dev = x.device
        held = self._pheld.get(k)
        held = held() if held is not None else None
        if held is not None:
            held.detach()  # a live result of the call two back: copy it out of the slot before the slot is rewritten
        per = 3 * self.h * self.w * 4
        ptrs = [x.data_ptr() + a * per for a, _ in self.bounds]
        if ptrs != self._slot_ptrs.get(k):  # (the words keep their value from call to call for the same tensor)
            self.bind_ptrs[k].copy_(torch.tensor(ptrs, dtype=torch.int64), non_blocking=True)
            self._slot_ptrs[k] = ptrs
        g = self._pgraph.get(k)
        if g is None:
            if self.fp8 and not self.fp8_ready:
                self.calibrate_fp8(calibration=self.fp8_calibration)
            if k not in self._max_work:
                self._max_work[k] = _lib.batch_max_work(dev)
            det, count, flat = _det_count(self.batch, self.max_det, dev)
            scale = torch.empty(1, dtype=torch.float32, device=dev)
            self._pout[k] = (det, count, flat, scale)
            pre = Plan(dev, self.dtype)
            pre.launch("ydbl_batch_max_bound", self.bind_ptrs[k, 0:1].data_ptr(), x.numel(), self._max_work[k].data_ptr(),
                       self.bind_amax[k].data_ptr(), scale.data_ptr(), what="LoadTensor.max")
            self._set_slot(k, det, count)
            if self.use_graph:
                g = (BranchGraphRunner(self.plans, pre=pre) if self.children else GraphRunner(self.plan, pre=pre))
            else:
                g = _EagerSlot(self, k, pre)
            self._set_slot(0)
            self._pgraph[k] = g
        cur = torch.cuda.current_stream(dev)
        if self._last_stream is not None and cur != self._last_stream:  # another stream: the last replay first
            cur.wait_event(self._slot_ev[1 + self._calls % 2])  # (the other slot's event: the previous call)
        g.replay()
        ev = self._slot_ev.get(k)
        if ev is None:
            ev = self._slot_ev[k] = torch.cuda.Event()
        ev.record(cur)
        self._last_stream = cur
        det, count, flat, scale = self._pout[k]
        out = BoundOutputs(det, count, flat, scale, ev)
        self._pheld[k] = weakref.ref(out)
        self._bound = x
        return out

    def calibrate_fp8(self, x: torch.Tensor | None = None, fraction: float | None = None, calibration=None) -> int:
        """Switch the dense convs to e4m3 operands (ydbl.quant).  calibration (an ydbl.quant.Fp8Calibration or the
        path of one saved with .save()): its activation scales, bias corrections and layer set; else one measured
        now on `x` (default: the batch already loaded) -- kept as self.fp8_calibration, .save() it to reuse.
        fraction < 1: only that share of the candidates' MACs, least output-sensitive convs first (default: the
        session's fp8_fraction).  Returns the number of convs switched."""
        from ..quant import Fp8Calibration, enable_fp8

        if self.sparse_box:
            raise RuntimeError("calibrate_fp8() on a sparse_box session: the calibration reads feats(), whose box logits "
                               "outside candidate tiles are not computed; build the session with fp8=...")
        if isinstance(calibration, (str, bytes)) or hasattr(calibration, "__fspath__"):
            calibration = Fp8Calibration.load(calibration)
        if x is not None and calibration is None:
            self.load(x)
        frac = self.fp8_fraction if fraction is None else float(fraction)
        # one joint calibration over every sub-batch plan (ydbl.quant.enable_fp8): the same activation scales
        # and the same fp8 layer set for every image of the batch, whichever stream it runs on
        parts = self.parts

        def run_all():
            for p in self.plans:
                p.run()

        def heads():
            return [t for c in parts for t in c.compiled.feats()]

        n = enable_fp8(self.plans, run_all, fraction=frac, head=heads, calibration=calibration)
        self.fp8_calibration = self.plan.fp8_calibration
        for c in (self, *parts):  # descriptors changed: recapture
            c._graph, c.fp8_ready = None, True
        self._pgraph.clear()
        return n

    @property
    def fp8_mac_fraction(self) -> float | None:
        """Share of the fp8 candidates' MACs switched to e4m3 (None before calibration)."""
        return getattr(self.plan, "fp8_mac_fraction", None)

    def outputs(self):
        return self.det, self.count

    def results(self):
        """Host list of [n_i, 6] tensors (one sync)."""
        cnt = self.count.cpu().tolist()
        det = self.det.cpu()
        return [det[i, : cnt[i]].clone() for i in range(self.batch)]

    def feats(self):
        """Per-level head maps [B, 64+nc, H_i, W_i]: NCHW views of the plan's level buffers (no copy); a split
        session concatenates its sub-batch plans' maps (a copy).

        A sparse_box session does NOT compute the box logits (channels 0..63) of its P3 / P4 maps outside the 8 x 16
        tiles that hold an NMS candidate: there the buffers keep whatever an earlier batch left.  The class logits and
        the 20^2 level are complete.  The call warns about it; for full maps build the session with keep_pred=True
        or under YDBL_NO_SPARSE_BOX=1."""
        if self.sparse_box:
            warnings.warn("feats() of a sparse_box session: box logits outside the tiles that hold an NMS candidate "
                          "are not computed (keep_pred=True or YDBL_NO_SPARSE_BOX=1 give full maps)", stacklevel=2)
        if self.children:
            per = [c.compiled.feats() for c in self.children]
            return [torch.cat([f[i] for f in per]) for i in range(len(per[0]))]
        return self.compiled.feats()


# Test-time augmentation (DetectionModel._predict_augment, U/nn/tasks.py:361-376): (ratio, left-right flip) per pass
AUG_PASSES = ((1.0, False), (0.83, True), (0.67, False))


def augment_passes(h: int, w: int, strides) -> list:
    """The three passes of augmented inference on an (h, w) input, as pure host arithmetic: per pass
    ``(ratio, flip, (sh, sw), (hp, wp), A, a_lo, a_hi, pos_base)`` -- scale_img's resized and padded sizes
    (preprocess.scale_img_shape, gs = the largest stride), the pass's anchor count A over ``strides``, the window
    [a_lo, a_hi) of its anchors that _clip_augmented keeps (U/nn/tasks.py:389-398: with g = sum(4**k, k < nl) the
    first pass loses its last A // g anchors -- its coarsest level at a square-ish size --, the last pass its first
    (A // g) * 4**(nl - 1) -- its finest), and the position of a_lo on the concatenated anchor axis."""
    from .preprocess import scale_img_shape

    strides = [int(s) for s in strides]
    nl, gs = len(strides), max(strides)
    g = sum(4 ** k for k in range(nl))
    out, pos = [], 0
    for i, (ratio, flip) in enumerate(AUG_PASSES):
        (sh, sw), (hp, wp) = ((h, w), (h, w)) if ratio == 1.0 else scale_img_shape(h, w, ratio, gs)
        A = sum((hp // s) * (wp // s) for s in strides)
        a_lo, a_hi = 0, A
        if i == 0:
            a_hi = A - A // g
        if i == len(AUG_PASSES) - 1:
            a_lo = (A // g) * 4 ** (nl - 1)
        out.append((ratio, flip, (sh, sw), (hp, wp), A, a_lo, a_hi, pos))
        pos += a_hi - a_lo
    return out


class AugmentSession(DetectSession):
    """``augment=True``: the reference's multi-scale + flip test-time augmentation as one launch plan.  Three compiled
    forwards at the shapes of augment_passes() share one candidate list, one det | count output and (keep_pred) one
    merged ``pred [B, 4+nc, A_tot]``:

        load() -> pass 0's staging buffer (LoadTensor-scaled, the copy path)
        ydbl_scale_img x 2            pass 0's staging buffer -> the staging buffers of passes 1 and 2
        per pass: forward, ydbl_detect_decode_aug   (de-scale, de-flip, anchor window, merged position; pass 0
                                                     zeroes the candidate counters, passes 1 and 2 append)
        ydbl_nms                      once, over the union, clipping to the original (h, w)

    all on one stream, captured as one hipGraph (use_graph): no host round trip between the passes.  streams = k
    splits the batch as DetectSession does, each sub-batch running its own three passes as one branch of the graph.
    Takes DetectSession's settings (DetectOptions).  Not supported, and refused as such: in-place input binding
    (can_bind() is False, so predict() takes the copy path, and launch_bound() raises ValueError), fp8 (the
    calibration is per compiled plan: NotImplementedError from the constructor and from calibrate_fp8()) and loss
    (the three passes have no single set of levels to score: ValueError from the constructor, and load_labels()
    raises RuntimeError as on any session built without loss=).  The NMS candidate capacity is A_tot (x nc
    multi-label): 15 049 at 640^2, above ydbl_nms's 8192-candidate pair-matrix limit like the plain session's 8400,
    so its workspace per image is the same ~9.1 MB (tail.nms_workspace: 16384 sort slots, 8 class-group lists, 8192
    pair-matrix rows)."""

    def __init__(self, model, batch: int, h: int, w: int, *args, device="cuda", streams=1, options=None,
                 _outputs=None, **kw):
        opt = _options(options, args, kw)
        if opt.fp8:
            raise NotImplementedError("augment=True with fp8: the fp8 calibration is per compiled plan, and the "
                                      "augmented session runs three; use half=True")
        if opt.loss is not None:
            raise ValueError("augment=True with loss: the three augmented passes have no single set of levels to score")
        self._init_detect(model, batch, h, w, opt, device, streams)
        self.passes = augment_passes(h, w, model.model[-1].stride.tolist())
        self.A = self.passes[-1][7] + self.passes[-1][6] - self.passes[-1][5]
        if _outputs is not None:  # slices of a split session's shared outputs
            self.det, self.count, self.pred = _outputs
        else:
            self._alloc_outputs(self.A)
        self._build()

    def _child(self, i: int, a: int, b: int):
        outs = (self.det[a:b], self.count[a:b], self.pred[a:b] if self.pred is not None else None)
        return AugmentSession(self.model, b - a, self.h, self.w, device=self.device, options=self.opt, _outputs=outs)

    def _compile(self) -> Plan:
        from .preprocess import SCALE_IMG_PAD

        batch, h, w, dev, A = self.batch, self.h, self.w, self.device, self.A
        cms = [self.model.compile(batch, hp, wp, self.dtype, device=dev) for _, _, _, (hp, wp), *_ in self.passes]
        self.compiled_passes, self.compiled = cms, cms[0]  # (load() fills pass 0's staging buffer)
        plan = Plan(dev, self.dtype)
        tail = self.tail = NmsTail(plan, batch, A, self.model.model[-1], self.opt, self.det, self.count, self.pred,
                                   segment=self.segment)
        ch = cms[0].input.shape[1]
        for cm, (ratio, flip, (sh, sw), (hp, wp), *_) in zip(cms[1:], self.passes[1:]):
            sd = ScaleImgDesc(cms[0].input.data_ptr(), batch, ch, h, w, sh, sw, hp, wp, int(flip), SCALE_IMG_PAD,
                              cm.input.data_ptr())
            plan.launch("ydbl_scale_img", sd, what=f"scale_img {ratio}", keep=[sd])
        for i, (cm, (ratio, flip, _, _, A_i, a_lo, a_hi, pos)) in enumerate(zip(cms, self.passes)):
            if sum(lv.h * lv.w for lv in cm.levels) != A_i:
                raise RuntimeError(f"pass {i}: the compiled levels hold {sum(lv.h * lv.w for lv in cm.levels)} "
                                   f"anchors, augment_passes() expects {A_i}")
            plan.steps += cm.plan.steps
            tail.emit_decode_aug(cm.levels, DecodeAug(float(ratio), float(w) if flip else 0.0, a_lo, a_hi, pos, A,
                                                      int(i > 0)), i)
        tail.emit_nms(h, w)
        return plan

    def can_bind(self, x) -> bool:
        """Never: scale_img reads pass 0's staging buffer, so predict() takes the copy path."""
        return False

    def calibrate_fp8(self, *a, **k):
        raise NotImplementedError("augment=True has no fp8 path (the calibration is per compiled plan)")

    def feats(self):
        """None: the reference's augmented forward returns (y, None) (U/nn/tasks.py:376)."""
        return None


class E2EForwardSession(BatchSession):
    """DetectionModel.forward on an end2end (YOLOv10) model: the forward with the head's whole inference forward
    behind it (v10Detect._forward_plan: one2many and one2one branches, the one2one decode, the top-k with no
    threshold and no clipping), one plan, one graph.  outputs(): (y [B, min(300, A), 6], {"one2many": [...],
    "one2one": [...]}) as fresh tensors of the session's dtype."""

    def __init__(self, model, batch: int, h: int, w: int, dtype=torch.float16, device="cuda", use_graph=True):
        super().__init__(model, batch, h, w, dtype, use_graph, device, 1)
        self._build()

    def _compile(self) -> Plan:
        cm = self.compiled = self.model.compile(self.batch, self.h, self.w, self.dtype, device=self.device,
                                                head_forward=True)
        return cm.plan

    def outputs(self):
        return self.compiled.finish()


class EmbedSession(BatchSession):
    """``embed=[i, ...]``: pooled layer features instead of detections (Model.embed, U/engine/model.py:467-499;
    _predict_once's early return, U/nn/tasks.py:158-171).  The compiled plan stops at layer max(embed) -- no Detect
    branches, no decode, no NMS -- with one ydbl_global_avgpool behind each named layer; ``out [B, D]`` (D = the
    layers' channel counts summed, ascending layer order, plan dtype) is owned by the session and rewritten by the
    next call.

    streams = k > 1 splits the batch into k contiguous sub-batches (BatchSession, as DetectSession): one plan per
    sub-batch, each writing its rows of the one shared ``out``, captured as the branches of ONE hipGraph
    (runtime.BranchGraphRunner); streams == 1 replays one GraphRunner.  Every plan passes Plan.check_single_stream.
    The batch goes through the staging copy (load(), with LoadTensor's /255 rule as its scale argument); there is no
    in-place input binding (launch_bound) for these sessions."""

    def __init__(self, model, batch: int, h: int, w: int, dtype=torch.float16, embed=None, device="cuda", streams=1,
                 use_graph=True, _out=None):
        from ..nn.tasks import _propagate_shapes, normalize_embed

        self.embed = normalize_embed(embed, len(model.model))
        super().__init__(model, batch, h, w, dtype, use_graph, device, streams)
        self.out = _out
        if len(self.bounds) > 1 and _out is None:  # one [B, D] output, each sub-batch plan compiled onto its row slice
            shapes = _propagate_shapes(list(model.model)[: self.embed[-1] + 1], 1, h, w, model.yaml["ch"])
            self.out = torch.empty((batch, sum(shapes[i][3] for i in self.embed)), dtype=dtype, device=self.device)
        self._build()
        self.dim = self.out.shape[1]

    def _child(self, i: int, a: int, b: int):
        return EmbedSession(self.model, b - a, self.h, self.w, self.dtype, self.embed, self.device,
                            use_graph=self.use_graph, _out=self.out[a:b])

    def _compile(self) -> Plan:
        cm = self.compiled = self.model.compile(self.batch, self.h, self.w, self.dtype, device=self.device,
                                                embed=self.embed, embed_out=self.out)
        self.out = cm.embed_out
        cm.plan.check_single_stream()
        return cm.plan

    def outputs(self) -> torch.Tensor:
        return self.out
