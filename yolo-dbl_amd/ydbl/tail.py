"""The detection tail: what stands between a head's level buffers [B, h, w, 4 * reg_max + nc] and det | count.

CandidateLists are the five tensors every descriptor of the tail names; decode_desc() builds the DecodeDesc of one
forward's levels; NmsTail (decode, or candidates from the class-conv tails, then ydbl_nms) and E2ETail (an end2end
head: decode_e2e, then ydbl_detect_topk) append their launches to a plan.  Imports only _lib and runtime, so the
heads (nn.modules), the sessions (engine.session) and utils.ops all build their tails here.
"""

from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from ._lib import DecodeDesc, NmsDesc, PoseKptDesc, TopkDesc, View
from .runtime import Plan

# Score threshold from which the NMS runs one workgroup per image instead of the class-split sweep (ydbl_nms_desc
# per_image): at predict-like thresholds every image has at most 1024 candidates (the pair-matrix path; DBL-n bs32
# at conf 0.25: 645 at most) and the split's extra workgroups and merge cost +0.8 % of the step
# (profiles/r05/r05_nms_per_image_ab.txt); validation's conf 0.001 keeps the split.
PER_IMAGE_NMS_CONF = 0.1


class CandidateLists:
    """The candidate lists a decode fills and an NMS / top-k reads (include/ydbl.h): box [B, cap, 4] fp32, score
    [B, cap] fp32, cls and idx [B, cap] int32, count [B] int32 (zero-filled), registered in plan.buffers when a plan
    is given."""

    def __init__(self, batch: int, cap: int, device, plan: Plan | None = None):
        self.cap = cap
        self.box = torch.empty((batch, cap, 4), dtype=torch.float32, device=device)
        self.score = torch.empty((batch, cap), dtype=torch.float32, device=device)
        self.cls = torch.empty((batch, cap), dtype=torch.int32, device=device)
        self.idx = torch.empty((batch, cap), dtype=torch.int32, device=device)
        self.count = torch.zeros((batch,), dtype=torch.int32, device=device)
        if plan is not None:
            plan.buffers += [self.box, self.score, self.cls, self.idx, self.count]

    @staticmethod
    def capacity(A: int, nc: int, multi_label) -> int:
        """Candidates per image of A anchors: one per anchor, one per (anchor, class) pair multi-label."""
        return A * nc if multi_label and nc > 1 else A

    def fields(self) -> dict:
        """The six fields DecodeDesc, PredCandDesc, NmsDesc and TopkDesc share, by their names there."""
        return dict(cand_box=self.box.data_ptr(), cand_score=self.score.data_ptr(), cand_cls=self.cls.data_ptr(),
                    cand_idx=self.idx.data_ptr(), cand_count=self.count.data_ptr(), cap=self.cap)


def decode_desc(levels, strides, nc, reg_max, conf, multi_label, classes, pred, cands: CandidateLists) -> DecodeDesc:
    """The decode of one forward's levels (box logits | class logits per level, strides = the head's) into `cands`
    and, if given, the prediction tensor pred [B, 4 + nc, A]; classes: a device int32 tensor or None."""
    boxes = (View * 3)(*[lv.cslice(0, 4 * reg_max).struct() for lv in levels])
    clss = (View * 3)(*[lv.cslice(4 * reg_max, nc).struct() for lv in levels])
    st = (C.c_float * 3)(*[float(s) for s in strides])
    return DecodeDesc(boxes, clss, len(levels), nc, st, float(conf), int(multi_label),
                      classes.data_ptr() if classes is not None else None, len(classes) if classes is not None else 0,
                      pred.data_ptr() if pred is not None else None, **cands.fields())


def nms_workspace(batch: int, cap: int, max_nms: int, device) -> torch.Tensor:
    """ydbl_nms's workspace for `batch` lists of `cap` candidates, zero-filled once (include/ydbl.h)."""
    return torch.zeros(int(_lib.lib.ydbl_nms_workspace(batch, cap, max_nms)), dtype=torch.uint8, device=device)


class _Tail:
    """What the two tails share: built over `plan` for `batch` images of A anchors behind `head` (nc, reg_max,
    stride) from the options record `opt` (engine.session.DetectOptions) and the caller's det [B, max_det, 6] /
    count [B] (views with their own image stride are fine; None: allocated) / pred (or None).  Owns the candidate
    lists ``cands`` and the ``classes`` filter as a device tensor."""

    fused = sparse = False  # (NmsTail: the candidates come from the class-conv tails / the sparse box path runs)
    keep_idx = kpts = None

    def __init__(self, plan: Plan, batch: int, A: int, head, opt, det, count, pred, multi_label: bool):
        dev = plan.device
        self.plan, self.batch, self.A, self.head, self.opt, self.pred = plan, batch, A, head, opt, pred
        self.conf, self.max_det, self.multi_label = float(opt.conf), int(opt.max_det), multi_label
        self.cands = CandidateLists(batch, CandidateLists.capacity(A, head.nc, multi_label), dev, plan)
        self.cap = self.cands.cap
        cl = opt.classes
        self.classes = torch.tensor(list(cl), dtype=torch.int32, device=dev) if cl is not None else None
        self.det = det if det is not None else torch.zeros((batch, self.max_det, 6), dtype=torch.float32, device=dev)
        self.count = count if count is not None else torch.zeros((batch,), dtype=torch.int32, device=dev)
        plan.buffers += [t for t in (self.det, self.count, self.classes, pred) if t is not None]

    def decode_desc(self, levels, classes=None) -> DecodeDesc:
        """The decode of one forward's levels into the candidate lists (and ``pred``); classes: the filter, where the
        decode applies it."""
        h = self.head
        return decode_desc(levels, h.stride.tolist(), h.nc, h.reg_max, self.conf, self.multi_label, classes,
                           self.pred, self.cands)

    def _emit_select(self, name: str, what: str, desc, h: int, w: int, **own):
        """The launch behind the decode, `desc` = NmsDesc or TopkDesc (nms=False: none): the fields the two share --
        the lists, det / count with their image strides, the clip to (h, w), the schedule -- and the descriptor's
        `own`."""
        opt = self.opt
        if not opt.nms:
            return
        d = desc(n=self.batch, max_det=self.max_det, clip_w=float(w) if opt.clip else 0.0,
                 clip_h=float(h) if opt.clip else 0.0, out=self.det.data_ptr(), out_count=self.count.data_ptr(),
                 out_stride=self.det.stride(0), count_stride=self.count.stride(0), workspace=self.ws.data_ptr(),
                 per_image=int(self.conf >= PER_IMAGE_NMS_CONF), **self.cands.fields(), **own)
        self.plan.launch(name, d, what=what, keep=[d])


class NmsTail(_Tail):
    """Decode + ydbl_nms: cap = A candidates per image (x nc multi-label), the ``classes`` filter in the decode, the
    NMS workspace zero-filled once (include/ydbl.h) and, for a Segment head, ``keep_idx`` [B, max_det]: per kept row
    the candidate's index, which finds its mask coefficients (ydbl_nms_desc.out_idx).  A Pose head (pose=True) gets
    ``keep_idx`` too, and ``kpts`` [B, max_det, K, ndim] fp32 (or the caller's view): the kept rows' keypoints, decoded
    by one ydbl_pose_keypoints launch behind the NMS (emit_keypoints)."""

    def __init__(self, plan: Plan, batch: int, A: int, head, opt, det, count, pred=None, segment=False, pose=False,
                 kpts=None):
        super().__init__(plan, batch, A, head, opt, det, count, pred, bool(opt.multi_label) and head.nc > 1)
        self.ws = nms_workspace(batch, self.cap, opt.max_nms, plan.device)
        plan.buffers.append(self.ws)
        if segment or pose:
            self.keep_idx = torch.full((batch, self.max_det), -1, dtype=torch.int32, device=plan.device)
            plan.buffers.append(self.keep_idx)
        if pose:
            K, ndim = head.kpt_shape
            self.kpts = kpts if kpts is not None else torch.zeros((batch, self.max_det, K, ndim), dtype=torch.float32,
                                                                  device=plan.device)
            plan.buffers.append(self.kpts)

    def emit_decode(self, levels) -> DecodeDesc:
        """The candidates of one compiled forward, whose launches are already in the plan.  No decode pass when every
        level's class conv is the tail of a DWConv -> Conv1x1 launch (DBL-n, nc <= 4, fp16) and no prediction tensor
        is wanted: those launches emit the candidates themselves (fuse_candidates).  The sparse box path on top of
        that (predict thresholds, fp16 operands only: the fp8 calibration reads feats(), and below PER_IMAGE_NMS_CONF
        most tiles hold a candidate): sparse_box.  Returns the decode descriptor (the loss reads its views)."""
        opt = self.opt
        dd = self.decode_desc(levels, self.classes)
        self.fused = self.pred is None and self.fuse_candidates(levels, dd)
        self.sparse = bool(opt.loss is None and self.fused and opt.nms and not opt.fp8
                           and self.conf >= PER_IMAGE_NMS_CONF and not os.environ.get("YDBL_NO_SPARSE_BOX")
                           and self.sparse_box(levels, dd))
        if not self.fused:
            self.plan.launch("ydbl_detect_decode", dd, what="Detect.decode", keep=[dd])
        return dd

    def emit_decode_aug(self, levels, ga: _lib.DecodeAug, i: int):
        """Pass i of an augmented session (ydbl_detect_decode_aug: ga = its de-scale, de-flip, anchor window and
        merged position) into the one candidate list."""
        dd = self.decode_desc(levels, self.classes)
        self.plan.launch("ydbl_detect_decode_aug", dd, ga, what=f"Detect.decode pass {i}", keep=[dd, ga])

    def emit_nms(self, h: int, w: int):
        """ydbl_nms over the candidate lists into det / count, clipping to (h, w); nms=False: forward + decode only
        (DetectionModel.forward -> (y, feats))."""
        opt = self.opt
        self._emit_select("ydbl_nms", "NMS", NmsDesc, h, w, iou_thres=float(opt.iou), max_nms=int(opt.max_nms),
                          agnostic=int(bool(opt.agnostic)), max_wh=float(opt.max_wh),
                          out_idx=self.keep_idx.data_ptr() if self.keep_idx is not None else None)

    def emit_keypoints(self, views):
        """ydbl_pose_keypoints behind emit_nms: the raw keypoint maps `views` (plan.pose) at the anchors keep_idx
        names -> ``kpts`` (slots past the count zeroed).  nms=False: nothing to decode."""
        if not self.opt.nms:
            return
        h = self.head
        K, ndim = h.kpt_shape
        assert self.kpts.is_contiguous() and self.count.stride(0) == 1
        d = PoseKptDesc((View * 3)(*[v.struct() for v in views]), len(views), h.nc if self.multi_label else 0,
                        (C.c_float * 3)(*[float(s) for s in h.stride.tolist()]), self.keep_idx.data_ptr(),
                        self.count.data_ptr(), self.batch, self.max_det, K, ndim, self.kpts.data_ptr())
        self.plan.launch("ydbl_pose_keypoints", d, what="Pose.keypoints", keep=[d])

    def fuse_candidates(self, levels, dd: DecodeDesc) -> bool:
        """Point the candidate sinks of the plan's class-conv tail launches (include/ydbl.h, ydbl_dsconv_desc) at the
        decode descriptor's lists.  Only when the plan is fp16 and EVERY level's class logits are written by such a
        tail (in level order, after the level's box launch: Detect.emit); else nothing is touched and the caller
        keeps the decode launch.  The first level's launch zeroes the counters."""
        plan = self.plan
        if plan.dtype != torch.float16:
            return False
        tails = {}
        for st in plan.steps:
            if st.fn.__name__ == "ydbl_dsconv_nhwc" and st.args[0].tail_w:
                tails[st.args[0].tail_y.ptr] = st.args[0]
        descs = [tails.get(dd.cls[i].ptr) for i in range(len(levels))]
        if any(d is None for d in descs):
            return False
        a0 = 0
        for i, (lv, d) in enumerate(zip(levels, descs)):
            d.cand_box, d.cand_score, d.cand_cls = dd.cand_box, dd.cand_score, dd.cand_cls
            d.cand_idx, d.cand_count, d.cand_cap = dd.cand_idx, dd.cand_count, dd.cap
            d.conf_thres, d.multi_label = dd.conf_thres, dd.multi_label
            d.classes, d.nclasses = dd.classes, dd.nclasses
            d.level_stride, d.anchor0, d.box = dd.stride[i], a0, dd.box[i]
            d.zero_counts = int(i == 0)
            a0 += lv.h * lv.w
        return True

    def sparse_box(self, levels, dd: DecodeDesc) -> bool:
        """The sparse box path (include/ydbl.h: the deferred sink of ydbl_dsconv_desc, the tile mask and candidate
        sink of ydbl_bottleneck_desc), on the levels whose box branch is ONE ydbl_bottleneck_nhwc launch with pw = 1
        (emit_detect_box: DBL-n P3 / P4): the level's box launch moves behind its class tail, the tail flags the
        8 x 16 tiles that hold a candidate instead of decoding, and the box launch computes only those tiles and
        decodes the candidates' boxes.  One mask buffer for all such levels, zeroed by the launch that zeroes the
        counters.  The other levels (20^2: three generic convs) keep their order and today's sink.  False, with
        nothing touched, when no level qualifies."""
        plan = self.plan
        tails, boxes = {}, {}
        for k, st in enumerate(plan.steps):
            name = st.fn.__name__
            if name == "ydbl_dsconv_nhwc" and st.args[0].tail_w and st.args[0].cand_count:
                tails[st.args[0].tail_y.ptr] = k
            elif name == "ydbl_bottleneck_nhwc" and st.args[0].pw:
                boxes[st.args[0].y.ptr] = k
        picks = []
        for i, lv in enumerate(levels):
            kb, kt = boxes.get(dd.box[i].ptr), tails.get(dd.cls[i].ptr)
            if kb is not None and kt is not None and kb < kt:
                picks.append((i, kb, kt, -(-lv.w // 16), -(-lv.h // 8)))
        if not picks:
            return False
        sizes = [levels[i].n * tx * ty for i, _, _, tx, ty in picks]
        mask = torch.zeros(sum(sizes), dtype=torch.uint8, device=plan.device)
        plan.buffers.append(mask)
        self.tile_masks, off, after = {}, 0, {}
        for (i, kb, kt, tx, ty), size in zip(picks, sizes):
            self.tile_masks[i] = mask[off:off + size].view(levels[i].n, ty, tx)
            td, bd = plan.steps[kt].args[0], plan.steps[kb].args[0]
            td.tile_mask, td.mask_tiles_x, td.mask_tiles_img = mask.data_ptr() + off, tx, tx * ty
            bd.tile_mask = mask.data_ptr() + off
            bd.cand_box, bd.cand_idx, bd.cand_count, bd.cand_cap = dd.cand_box, dd.cand_idx, dd.cand_count, dd.cap
            bd.level_stride, bd.anchor0, bd.nc, bd.multi_label = td.level_stride, td.anchor0, dd.nc, dd.multi_label
            after[kt] = plan.steps[kb]
            off += size
        for st in plan.steps:  # the call that zeroes the counters zeroes the masks too
            if st.fn.__name__ == "ydbl_dsconv_nhwc" and st.args[0].cand_count and st.args[0].zero_counts:
                st.args[0].mask_zero, st.args[0].mask_zero_bytes = mask.data_ptr(), mask.numel()
        moved = {id(s) for s in after.values()}
        steps = []
        for k, st in enumerate(plan.steps):  # class branch first, the level's box launch right behind its tail
            if id(st) in moved:
                continue
            steps.append(st)
            if k in after:
                steps.append(after[k])
        plan.steps = steps
        return True


class E2ETail(_Tail):
    """The tail of an end2end head (v10Detect; U/nn/modules/head.py:120-141, :200-221 and the six-column branch of
    non_max_suppression, U/utils/ops.py:224-228) behind its one2one levels: ydbl_detect_decode_e2e in multi-label
    mode whatever opt.multi_label and nc are (cap = A * nc, xyxy boxes, score > conf; -1 = every pair,
    DetectionModel.forward; no `classes` filter), then ydbl_detect_topk where the NMS stands for the other heads --
    the first min(min(head.max_det, A), max_det) pairs by (score, anchor * nc + class), the `classes` filter behind
    the cut.  iou, agnostic, max_nms and max_wh play no part, as in the reference; no fused candidates, no sparse box
    path.  pred: the dense one2one map [B, 4+nc, A] with xyxy rows."""

    def __init__(self, plan: Plan, batch: int, A: int, head, opt, det=None, count=None, pred=None):
        super().__init__(plan, batch, A, head, opt, det, count, pred, True)
        nws = 16 if plan.device.type == "meta" else int(_lib.lib.ydbl_detect_topk_workspace(batch, self.cap))
        self.ws = torch.empty(nws, dtype=torch.uint8, device=plan.device)
        plan.buffers.append(self.ws)

    def emit_decode(self, levels) -> DecodeDesc:
        dd = self.decode_desc(levels)
        self.plan.launch("ydbl_detect_decode_e2e", dd, what="Detect.decode e2e", keep=[dd])
        return dd

    def emit_topk(self, h: int, w: int):
        """ydbl_detect_topk over the candidate lists into det / count, clipping to (h, w); nms=False: the decode
        alone."""
        cl = self.classes
        self._emit_select("ydbl_detect_topk", "TopK", TopkDesc, h, w, k_head=min(int(self.head.max_det), self.A),
                          classes=cl.data_ptr() if cl is not None else None, nclasses=len(cl) if cl is not None else 0,
                          workspace_bytes=self.ws.numel())
