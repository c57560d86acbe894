"""The detection loss on the device: ``v8DetectionLoss`` (U/utils/loss.py:157-260) over ydbl_detect_loss.

The TaskAlignedAssigner (U/utils/tal.py:40-295) and the CIoU / BCE / DFL terms in one C-ABI call (csrc/loss.hip)
that reads the Detect head's level maps in place; the numbers are the reference's ``val/box_loss``,
``val/cls_loss`` and ``val/dfl_loss``.  The criterion is differentiable: when a level map requires grad the call
goes through a ``torch.autograd.Function`` whose backward is one ydbl_detect_loss_grad launch (csrc/loss_grad.hip)
over the assignment the forward kept, so it can stand in for ``model.criterion`` in a PyTorch trainer.  The network
itself has no backward pass here.

Host-side pieces (pure torch on the CPU, usable without a GPU): ``loss_gains`` (hyp.box / cls / dfl),
``check_labels`` (the guards: capacity and class range, raised before anything is launched) and ``pad_targets``
(``preprocess``, loss.py:180-195, into the fixed-capacity ``gt [B, max_labels, 5]`` buffer the kernel reads).
"""

from __future__ import annotations

import ctypes as C

import torch

from .. import _lib

MAX_LABELS = 300  # default capacity of the label buffer, per image
DEFAULT_GAINS = {"box": 7.5, "cls": 0.5, "dfl": 1.5}  # U/cfg/default.yaml:99-101
TAL_TOPK_MAX = 16


def loss_gains(model) -> tuple:
    """(box, cls, dfl) from ``model.args`` -- a dict or a namespace, as the reference's ``self.hyp`` -- else the
    defaults of U/cfg/default.yaml:99-101."""
    h = getattr(model, "args", None)
    out = []
    for k, d in DEFAULT_GAINS.items():
        v = h.get(k) if isinstance(h, dict) else getattr(h, k, None)
        out.append(float(d if v is None else v))
    return tuple(out)


def check_labels(batch_idx, cls, batch_size: int, nc: int, max_labels: int = MAX_LABELS):
    """The host guards of the loss, before anything is launched: ValueError for an image index outside
    [0, batch_size), a class outside [0, nc) or an image with more than max_labels labels.  Returns
    (batch_idx int64 [N], cls fp32 [N]) on the CPU."""
    bi = torch.as_tensor(batch_idx).reshape(-1).cpu().long()
    cl = torch.as_tensor(cls).reshape(-1).cpu().float()
    if len(bi) != len(cl):
        raise ValueError(f"batch_idx holds {len(bi)} labels, cls {len(cl)}")
    if len(bi):
        if int(bi.min()) < 0 or int(bi.max()) >= batch_size:
            raise ValueError(f"batch_idx must be in [0, {batch_size})")
        if not bool(((cl >= 0) & (cl < nc)).all()):
            bad = cl[~((cl >= 0) & (cl < nc))][0].item()
            raise ValueError(f"label class {bad:g} is outside [0, {nc})")
        most = int(torch.bincount(bi, minlength=batch_size).max())
        if most > max_labels:
            raise ValueError(f"an image has {most} labels, the label buffer holds max_labels={max_labels} per image")
    return bi, cl


def pad_targets(batch_idx, cls, bboxes, batch_size: int, scale, max_labels: int = MAX_LABELS, xywh: bool = True,
                nc: int | None = None) -> torch.Tensor:
    """``preprocess`` (U/utils/loss.py:180-195) into a fixed capacity: CPU fp32 [batch_size, max_labels, 5], rows
    cls, x1, y1, x2, y2 in each image's own label order, zero-padded.  xywh=True: ``bboxes`` are normalised xywh,
    multiplied by ``scale`` = (w, h, w, h) and converted with xywh2xyxy's arithmetic (U/utils/ops.py:416-433);
    False: xyxy pixels, taken as they are.  Runs check_labels when ``nc`` is given."""
    if nc is not None:
        bi, cl = check_labels(batch_idx, cls, batch_size, nc, max_labels)
    else:
        bi = torch.as_tensor(batch_idx).reshape(-1).cpu().long()
        cl = torch.as_tensor(cls).reshape(-1).cpu().float()
    bb = torch.as_tensor(bboxes).reshape(-1, 4).cpu().float()
    if len(bb) != len(bi):
        raise ValueError(f"bboxes holds {len(bb)} labels, batch_idx {len(bi)}")
    out = torch.zeros((batch_size, max_labels, 5), dtype=torch.float32)
    if len(bi) == 0:
        return out
    if xywh:
        bb = bb * torch.as_tensor(scale, dtype=torch.float32).reshape(1, 4)
        xy, wh = bb[:, :2], bb[:, 2:] / 2
        bb = torch.cat((xy - wh, xy + wh), 1)
    order = torch.argsort(bi, stable=True)
    counts = torch.bincount(bi, minlength=batch_size)
    first = torch.cumsum(counts, 0) - counts
    rank = torch.arange(len(bi)) - first[bi[order]]
    out[bi[order], rank, 0] = cl[order]
    out[bi[order], rank, 1:] = bb[order]
    return out


def level_views(feats):
    """The head maps ``feats`` ([B, 64+nc, H_i, W_i] each, as DetectionModel.forward and DetectSession.feats() return
    them) as NHWC (box, cls) view records for ydbl_detect_loss, read in place where the memory is channels-last with
    a uniform pixel pitch (the session's own buffers), else from one channels-last copy.  Returns (boxes, clss,
    keep): two lists of _lib.View and the tensors they point into."""
    boxes, clss, keep = [], [], []
    for f in feats:
        if not isinstance(f, torch.Tensor) or f.ndim != 4 or f.shape[1] <= 64:
            raise TypeError("feats: a list of [B, 64+nc, H, W] tensors expected")
        if f.device.type != "cuda":
            raise RuntimeError(f"the detection loss runs on MI355X (gfx950) only: level maps on {f.device}")
        if f.dtype not in (torch.float16, torch.float32):
            f = f.float()
        b, c, h, w = f.shape
        sb, sc, sh, sw = f.stride()
        if not (sc == 1 and sw >= c and sh == w * sw and sb == h * sh):
            f = f.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # channels-last, pitch c
            sw = c
        keep.append(f)
        dt, es = _lib.dtype_code(f.dtype), f.element_size()
        boxes.append(_lib.View(f.data_ptr(), b, h, w, 64, sw, dt))
        clss.append(_lib.View(f.data_ptr() + 64 * es, b, h, w, c - 64, sw, dt))
    return boxes, clss, keep


class LossBuffers:
    """The device side of one ydbl_detect_loss call site: gt [B, max_labels, 5], loss [3], target_scores_sum [1],
    per_image [B, 3], the workspace and the descriptor over given level views.  debug=True adds the assignment
    (fg / target_gt_idx int32 [B, A], target_score fp32 [B, A])."""

    def __init__(self, boxes, clss, strides, nc: int, gains, max_labels: int = MAX_LABELS, topk: int = 10,
                 device="cuda", debug: bool = False, reg_max: int = 16):
        dev = torch.device(device)
        if not 1 <= int(topk) <= TAL_TOPK_MAX:
            raise ValueError(f"tal_topk must be in [1, {TAL_TOPK_MAX}]")
        B = boxes[0].n
        A = sum(v.h * v.w for v in boxes)
        meta = dev.type == "meta"
        self.batch, self.anchors, self.max_labels = B, A, int(max_labels)
        self.gt = torch.zeros((B, self.max_labels, 5), dtype=torch.float32, device=dev)
        self.out = torch.zeros(4 + 3 * B, dtype=torch.float32, device=dev)  # loss[3] | target_scores_sum | per_image
        self.loss, self.target_scores_sum, self.per_image = self.out[:3], self.out[3:4], self.out[4:].view(B, 3)
        need = int(_lib.lib.ydbl_detect_loss_workspace(B, A, self.max_labels))
        if need < 0:
            raise ValueError(f"ydbl_detect_loss_workspace({B}, {A}, {self.max_labels}) rejected its arguments")
        self.workspace = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        self.fg = self.target_gt_idx = self.target_score = None
        if debug:
            self.fg = torch.zeros((B, A), dtype=torch.int32, device=dev)
            self.target_gt_idx = torch.zeros((B, A), dtype=torch.int32, device=dev)
            self.target_score = torch.zeros((B, A), dtype=torch.float32, device=dev)
        d = _lib.LossDesc()
        for i, (bv, cv) in enumerate(zip(boxes, clss)):
            d.box[i], d.cls[i], d.stride[i] = bv, cv, float(strides[i])
        d.nl, d.nc, d.reg_max = len(boxes), int(nc), int(reg_max)
        d.max_labels, d.topk = self.max_labels, int(topk)
        d.gain_box, d.gain_cls, d.gain_dfl = (float(g) for g in gains)
        if not meta:
            ws = self.workspace.data_ptr()
            ws += -ws % 16
            d.gt = self.gt.data_ptr()
            d.loss, d.target_scores_sum = self.loss.data_ptr(), self.target_scores_sum.data_ptr()
            d.per_image = self.per_image.data_ptr()
            d.workspace, d.workspace_bytes = ws, need
            if debug:
                d.fg, d.target_gt_idx = self.fg.data_ptr(), self.target_gt_idx.data_ptr()
                d.target_score = self.target_score.data_ptr()
        self.desc = d

    def tensors(self):
        return [t for t in (self.gt, self.out, self.workspace, self.fg, self.target_gt_idx, self.target_score)
                if t is not None]

    def launch(self, stream=None):
        dev = self.gt.device
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream if stream is None else stream)
        _lib.check(_lib.lib.ydbl_detect_loss(C.byref(self.desc), s), "ydbl_detect_loss")


class v8DetectionLoss:
    """U/utils/loss.py:157-260 with the reference's call shape: ``criterion(preds, batch)`` -> ``(loss.sum() *
    batch_size, loss_items)`` as fp32 device tensors, without a host sync.  ``preds``: the ``feats`` list or the
    ``(y, feats)`` tuple of DetectionModel.forward; ``batch``: ``batch_idx [N]``, ``cls [N]`` or ``[N, 1]``,
    ``bboxes [N, 4]`` normalised xywh of the input.  After a call ``target_scores_sum`` and ``per_image`` hold the
    batch's normaliser and the [B, 3] per-image table (rows add up to loss_items).  With grad mode on and a level map
    that requires grad, the total carries a ``grad_fn`` (once differentiable; ``loss_items`` stays detached) and
    ``backward()`` delivers d(total)/d(level map) to every map; otherwise the call is the plain forward."""

    def __init__(self, model, tal_topk: int = 10, max_labels: int = MAX_LABELS):
        m = model.model[-1]  # Detect() module
        self.hyp = getattr(model, "args", None)
        self.gains = loss_gains(model)
        self.stride = [float(s) for s in m.stride.tolist()]
        self.nc, self.reg_max = m.nc, m.reg_max
        self.no = m.nc + m.reg_max * 4
        if m.reg_max != 16:
            raise NotImplementedError(f"the loss kernel is built for reg_max 16, the head has {m.reg_max}")
        if not 1 <= int(tal_topk) <= TAL_TOPK_MAX:
            raise ValueError(f"tal_topk must be in [1, {TAL_TOPK_MAX}]")
        self.tal_topk, self.max_labels = int(tal_topk), int(max_labels)
        self.target_scores_sum = self.per_image = None

    def preprocess(self, batch, batch_size: int, imgsz) -> torch.Tensor:
        """The padded label buffer of a reference batch dict for an (h, w) input (loss.py:180-195, :219-226); the
        guards of check_labels fire here."""
        h, w = imgsz
        return pad_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], batch_size, (w, h, w, h),
                           self.max_labels, nc=self.nc)

    def __call__(self, preds, batch):
        feats = preds[1] if isinstance(preds, tuple) else preds
        if feats is None:
            raise ValueError("preds holds no level maps (an augmented forward returns (y, None))")
        b, _, h0, w0 = feats[0].shape
        gt = self.preprocess(batch, b, (h0 * self.stride[0], w0 * self.stride[0]))  # host guards first
        if torch.is_grad_enabled() and any(isinstance(f, torch.Tensor) and f.requires_grad for f in feats):
            total, items = _DetectionLossFn.apply(self, gt, *feats)
            return total, items
        boxes, clss, keep = level_views(feats)
        dev = keep[0].device
        with torch.cuda.device(dev):
            bufs = LossBuffers(boxes, clss, self.stride, self.nc, self.gains, self.max_labels, self.tal_topk, dev)
            bufs.gt.copy_(gt, non_blocking=True)
            bufs.launch()  # (same stream as the allocations: the caching allocator keeps the order)
        self.target_scores_sum, self.per_image = bufs.target_scores_sum, bufs.per_image
        return bufs.loss.sum() * b, bufs.loss


# pitch of the gradient buffers in elements, rounded up to this: dense (the kernel's 16-byte stores need element
# alignment only)
GRAD_PITCH_ALIGN = 1


class LossGradBuffers:
    """The device side of one ydbl_detect_loss_grad call: per level one channels-last gradient buffer [B, H, W, pitch]
    in the level's dtype (pitch: 64 + nc rounded up to ``pitch_align`` elements; dense by default) and the descriptor
    over
    the channels-last level tensors ``keep`` (level_views), the label buffer ``gt`` and the assignment the forward
    wrote.  ``grad_scale``: a device fp32 scalar (the upstream gradient of the total) or None for 1."""

    def __init__(self, keep, strides, nc: int, gains, gt, fg, target_gt_idx, target_score, target_scores_sum,
                 batch_scale: float, grad_scale=None, pitch_align: int = GRAD_PITCH_ALIGN):
        d = _lib.LossGradDesc()
        d.nl, d.nc, d.reg_max, d.max_labels = len(keep), int(nc), 16, int(gt.shape[1])
        d.gain_box, d.gain_cls, d.gain_dfl = (float(g) for g in gains)
        d.gt, d.fg, d.target_gt_idx = gt.data_ptr(), fg.data_ptr(), target_gt_idx.data_ptr()
        d.target_score, d.target_scores_sum = target_score.data_ptr(), target_scores_sum.data_ptr()
        d.batch_scale = float(batch_scale)
        if grad_scale is not None:
            d.grad_scale = grad_scale.data_ptr()
        self.grads = []
        for i, f in enumerate(keep):
            b, c, h, w = f.shape
            pitch = -(-c // pitch_align) * pitch_align
            g = torch.empty((b, h, w, pitch), dtype=f.dtype, device=f.device)
            self.grads.append(g)
            dt, es, sw = _lib.dtype_code(f.dtype), f.element_size(), f.stride(3)
            d.box[i] = _lib.View(f.data_ptr(), b, h, w, 64, sw, dt)
            d.cls[i] = _lib.View(f.data_ptr() + 64 * es, b, h, w, c - 64, sw, dt)
            d.gbox[i] = _lib.View(g.data_ptr(), b, h, w, 64, pitch, dt)
            d.gcls[i] = _lib.View(g.data_ptr() + 64 * es, b, h, w, c - 64, pitch, dt)
            d.stride[i] = float(strides[i])
        self.channels = [f.shape[1] for f in keep]
        self.desc, self.keep = d, (keep, gt, fg, target_gt_idx, target_score, target_scores_sum, grad_scale)

    def launch(self, stream=None):
        dev = self.grads[0].device
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream if stream is None else stream)
        _lib.check(_lib.lib.ydbl_detect_loss_grad(C.byref(self.desc), s), "ydbl_detect_loss_grad")

    def views(self):
        """The gradients as [B, 64+nc, H, W] views of the channels-last buffers."""
        return [g[..., :c].permute(0, 3, 1, 2) for g, c in zip(self.grads, self.channels)]


class _DetectionLossFn(torch.autograd.Function):
    """``criterion(feats, batch)`` with a backward: the forward is the same ydbl_detect_loss call with the assignment
    kept, the backward one ydbl_detect_loss_grad launch.  The assignment, the labels and target_scores_sum are
    constants, as in the reference (U/utils/loss.py:233-243); ``loss_items`` carries no gradient (``loss.detach()``,
    :260)."""

    @staticmethod
    def forward(ctx, crit, gt, *feats):
        boxes, clss, keep = level_views(feats)
        dev = keep[0].device
        b = boxes[0].n
        with torch.cuda.device(dev):
            bufs = LossBuffers(boxes, clss, crit.stride, crit.nc, crit.gains, crit.max_labels, crit.tal_topk, dev,
                               debug=True)
            bufs.gt.copy_(gt, non_blocking=True)
            bufs.launch()
            total = bufs.loss.sum() * b
        crit.target_scores_sum, crit.per_image = bufs.target_scores_sum, bufs.per_image
        ctx.save_for_backward(*keep, bufs.gt, bufs.fg, bufs.target_gt_idx, bufs.target_score, bufs.target_scores_sum)
        ctx.crit, ctx.nl, ctx.batch = crit, len(keep), b
        ctx.in_dtypes = [f.dtype for f in feats]
        ctx.mark_non_differentiable(bufs.loss)
        return total, bufs.loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, _g_items):
        crit, nl = ctx.crit, ctx.nl
        saved = ctx.saved_tensors
        keep, assignment = saved[:nl], saved[nl:]
        dev = keep[0].device
        with torch.cuda.device(dev):
            scale = g_total.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
            gb = LossGradBuffers(keep, crit.stride, crit.nc, crit.gains, *assignment, float(ctx.batch), scale)
            gb.launch()  # (same stream as the allocations: the caching allocator keeps the order)
        grads = [g if g.dtype == dt else g.to(dt) for g, dt in zip(gb.views(), ctx.in_dtypes)]
        return (None, None, *grads)
