"""User API: ``YOLO(cfg_or_weights)`` with ``.predict()``, ``.track()``, ``.embed()``, ``.val()``, ``.fuse()``.

Mirrors U/engine/model.py:84-643 and U/models/yolo/model.py:52-100 for the
detect task: model files named like the reference's
(``yolov13n_DBL.yaml`` / ``yolov13s_DBL.yaml`` / ``yolov13l_DBL2.yaml``) build
the same layer graph; ``predict`` keeps the reference's argument names and
defaults (conf 0.25, iou 0.7, max_det 300, half False, agnostic_nms, classes;
U/cfg/default.yaml:51-54 and U/engine/model.py:547) and returns ``Results``.
Everything after construction runs on the GPU through libydbl; there is no CPU
execution path (``device='cpu'`` raises).
"""

from __future__ import annotations

import operator
import time
from collections import OrderedDict
from dataclasses import fields
from pathlib import Path

import numpy as np
import torch

from ..nn.tasks import DetectionModel, normalize_embed, weights_signature, ydbl_env
from .results import Results
from .session import (AugmentSession, DetectOptions, DetectSession, EmbedSession, check_pose, check_segment,
                      default_streams)

DEFAULTS = {"conf": 0.25, "iou": 0.7, "max_det": 300, "half": False, "fp8": False, "device": None, "agnostic_nms": False,
            "classes": None, "batch": 1, "verbose": False, "imgsz": 640,
            # sub-batch graphs per session (DetectSession): None = default_streams(batch), the benched layout
            "streams": None,
            # fp8: an ydbl.quant.Fp8Calibration or its JSON file (None: calibrate on the first batch)
            "fp8_calibration": None,
            # test-time augmentation (U/nn/tasks.py:361-398): three passes (1, 0.83 flipped, 0.67), one NMS
            "augment": False,
            # layer indices whose pooled outputs predict() returns instead of Results (U/cfg/default.yaml:67)
            "embed": None,
            # segmentation models: masks at the original image's size, cropped after the resampling
            # (process_mask_native, U/cfg/default.yaml:66); mask_dtype (ours): torch.uint8 keeps Masks.data as bytes
            # instead of the reference's fp32 0 / 1
            "retina_masks": False, "mask_dtype": None}


def check_augment(augment, fp8=False, gather_rows=None) -> bool:
    """augment's scope guards, before any device work: no fp8 (its calibration is per compiled plan; the augmented
    session runs three) and no record rows of the batch-sharded predictor."""
    if augment and fp8:
        raise NotImplementedError("augment=True with fp8 is not implemented: the fp8 calibration is per compiled "
                                  "plan and the augmented session runs three; use half=True")
    if augment and gather_rows is not None:
        raise NotImplementedError("augment=True is not implemented for the batch-sharded predictor (gather_rows)")
    return bool(augment)


def check_embed(embed, n_layers: int, augment=False, fp8=False, gather_rows=None):
    """embed's guards, before any device work: the normalised layer tuple (nn.tasks.normalize_embed; ValueError for
    an index outside [0, n_layers - 2] or a non-integer), or None when no embedding is asked for.  augment=True has
    no embedding (the reference silently ignores embed there: ValueError); fp8 and the batch-sharded predictor's
    record rows are not implemented for it."""
    if embed is None or (isinstance(embed, (list, tuple)) and not embed):
        return None
    embed = normalize_embed(embed, n_layers)
    if augment:
        raise ValueError("embed with augment=True: the augmented forward returns no embedding (the reference "
                         "silently ignores embed there); drop one of the two")
    if fp8:
        raise NotImplementedError("embed with fp8 is not implemented; use half=True")
    if gather_rows is not None:
        raise NotImplementedError("embed is not implemented for the batch-sharded predictor (gather_rows)")
    return embed


def check_loss(loss, augment=False, gather_rows=None):
    """loss's scope guards, before any device work: the augmented forward runs three passes and has no single set of
    levels to score (ValueError); the batch-sharded predictor's shards would each normalise by their own target
    scores (NotImplementedError).  Returns the session's loss settings (a dict) or None."""
    if not loss:
        return None
    if augment:
        raise ValueError("loss=True with augment=True: the three augmented passes have no single set of levels to "
                         "score; drop one of the two")
    if gather_rows is not None:
        raise NotImplementedError("loss=True is not implemented for the batch-sharded predictor (gather_rows)")
    return dict(loss) if isinstance(loss, dict) else {}


def select_device(device=None) -> torch.device:
    """U/utils/torch_utils.py select_device, GPU-only."""
    if device is None or device == "":
        device = 0
    if isinstance(device, torch.device):
        dev = device
    elif isinstance(device, int):
        dev = torch.device("cuda", device)
    else:
        s = str(device).lower().replace("cuda:", "").strip()
        if s == "cpu":
            raise RuntimeError("ydbl runs on MI355X (gfx950) only; device='cpu' has no implementation")
        dev = torch.device("cuda", int(s.split(",")[0]) if s else 0)
    if dev.type != "cuda":
        raise RuntimeError(f"ydbl runs on MI355X (gfx950) only; got device {dev}")
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: ydbl has no CPU fallback")
    return dev


def load_tensor_source(im: torch.Tensor, stride: int = 32) -> torch.Tensor:
    """LoadTensor._single_check (U/data/loaders.py:515-580): BCHW, H and W divisible by the stride, /255 if >1."""
    im = check_tensor_source(im, stride)
    if im.max() > 1.0 + torch.finfo(im.dtype).eps:
        im = im.float() / 255.0
    return im


def check_tensor_source(im, stride: int = 32) -> torch.Tensor:
    """The shape rules of LoadTensor._single_check (no device work): a BCHW tensor (or a list of CHW / 1CHW)."""
    if isinstance(im, (list, tuple)):
        im = torch.stack([t if t.ndim == 3 else t[0] for t in im])
    if not isinstance(im, torch.Tensor):
        raise TypeError(f"ydbl predict() takes torch tensors (BCHW float); got {type(im).__name__}")
    if im.ndim == 3:
        im = im.unsqueeze(0)
    if im.ndim != 4 or im.shape[1] != 3:
        raise ValueError(f"torch.Tensor inputs should be BCHW i.e. shape(b, 3, h, w) but got {tuple(im.shape)}")
    if im.shape[2] % stride or im.shape[3] % stride:
        raise ValueError(
            f"torch.Tensor inputs should be BCHW with height and width divisible by stride {stride}; got {tuple(im.shape)}")
    return im


_SCALES = {}


def _calib_key(cal):
    """Session-cache key of an fp8 calibration: its path, or a fingerprint of its content (not id(): a new object
    for the same record would compile a new session, and a recycled id could hit a session of another record)."""
    if cal is None or isinstance(cal, (str, Path)):
        return None if cal is None else str(cal)
    fp = getattr(cal, "_ydbl_fingerprint", None)
    if fp is None:
        import hashlib
        import json

        fp = hashlib.sha1(json.dumps(cal.to_json(), sort_keys=True).encode()).hexdigest()
        try:
            cal._ydbl_fingerprint = fp
        except AttributeError:
            pass
    return fp


_OPTION_NAMES = tuple(f.name for f in fields(DetectOptions))
_OPTION_VALUES = operator.attrgetter(*_OPTION_NAMES)
_I_CALIB, _I_LOSS = _OPTION_NAMES.index("fp8_calibration"), _OPTION_NAMES.index("loss")


def session_key(opt: DetectOptions, batch, h, w, dev, streams, gather_rows=None, augment=False) -> tuple:
    """Session-cache key of a detection session: the shape, EVERY field of its options record (the calibration by
    _calib_key, the loss settings by their sorted items), the placement and the YDBL_* switches -- those (plan-builder
    fusions in ydbl.nn.modules; YDBL_DS_LEAN / YDBL_NMS_* in the C-ABI) are read at plan build or at each launch, so
    a captured graph keeps the routing of its capture: a different switch setting is a different session."""
    o = list(_OPTION_VALUES(opt))
    o[_I_CALIB] = _calib_key(o[_I_CALIB])
    if o[_I_LOSS] is not None:
        o[_I_LOSS] = tuple(sorted((k, str(v)) for k, v in o[_I_LOSS].items()))
    return (batch, h, w, *o, str(dev), int(streams), gather_rows, augment, ydbl_env())


def _scale_consts(dev):
    """(1.0, fp32(1/255)) as 0-dim fp32 tensors on `dev` (made once)."""
    c = _SCALES.get(dev)
    if c is None:
        c = _SCALES[dev] = (torch.ones((), dtype=torch.float32, device=dev),
                            torch.full((), 1.0 / 255.0, dtype=torch.float32, device=dev))
    return c


def _load_tensor_scale(im: torch.Tensor) -> torch.Tensor:
    """LoadTensor's /255 rule for a device batch, without a host sync: fp32(1/255) when its maximum is > 1, else 1."""
    one, inv = _scale_consts(im.device)
    thr = 1.0 + (torch.finfo(im.dtype).eps if im.is_floating_point() else 0.0)
    return torch.where(im.amax() > thr, inv, one)


class _LazyHWC:
    """Per-image HWC views of a batch, scaled by a 0-dim device tensor, made on first access (Results.orig_img)."""

    def __init__(self, im, scale):
        self.im, self.scale, self.hwc = im, scale, None

    def __getitem__(self, i):
        if self.hwc is None:
            scale = self.scale() if callable(self.scale) else self.scale
            x = self.im.float() if scale is None else self.im.float() * scale
            self.hwc = x.permute(0, 2, 3, 1)
        return self.hwc[i]


class _LazyCounts:
    """The per-image detection counts of a batch, read to the host once, on first access: predict() returns without
    waiting for the GPU, and the batch's Results synchronise when one of them is first looked at.  cnt: the device
    tensor, or a callable producing it then (a session slot's outputs, copied out on first access)."""

    def __init__(self, cnt):
        self.cnt, self.host = cnt, None

    def __getitem__(self, i):
        if self.host is None:
            self.host = (self.cnt() if callable(self.cnt) else self.cnt).tolist()
        return self.host[i]


class Model:
    """U/engine/model.py:84-643 (detect task subset)."""

    def __init__(self, model: str | Path = "yolov13n_DBL.yaml", task=None, verbose=False, nc=None, kpt_shape=None):
        self.task = task or "detect"
        self.overrides = {}
        self.ckpt_path = None
        self.verbose = verbose
        self._sessions = OrderedDict()  # LRU of compiled sessions (each holds its own HBM buffers)
        self._trackers = {}  # track(persist=True): the device state of the ByteTrack trackers (engine.tracker)
        model = str(model)
        suffix = Path(model).suffix.lower()
        if suffix in (".pt", ".pth"):
            # reference checkpoint: build from its embedded yaml, then load its weights (U/nn/tasks.py:921-944)
            from ..utils.checkpoint import read_reference_checkpoint

            ck = read_reference_checkpoint(model)
            if ck["yaml"] is None:
                raise ValueError(f"{model} has no embedded model yaml: build from a config and call .load()")
            self.model = DetectionModel(ck["yaml"], nc=nc, verbose=verbose, data_kpt_shape=kpt_shape)
            self._load_sd(ck["state_dict"])
            if ck["names"]:
                self.model.names = ck["names"]
            self.ckpt_path = model
        elif suffix == ".safetensors":
            raise ValueError("build from a config and call .load(weights): YOLO('yolov13n_DBL.yaml').load('w.safetensors')")
        else:
            self.model = DetectionModel(model, nc=nc, verbose=verbose, data_kpt_shape=kpt_shape)
        if self.model.segment:  # U/nn/tasks.py guess_model_task: a Segment head is the "segment" task
            self.task = "segment"
        if self.model.pose:  # and a Pose head the "pose" task
            self.task = "pose"
        self.cfg = model
        self.overrides["model"] = model

    # ------------------------------------------------------------------ weights
    def load(self, weights):
        """Load a state_dict (torch weights_only file, safetensors, or a dict) with the reference's key names."""
        names = None
        if isinstance(weights, dict):
            sd = weights
        elif str(weights).endswith(".safetensors"):
            from safetensors.torch import load_file

            sd = load_file(str(weights))
        else:
            # plain state_dict files and the reference trainer's checkpoints, both without executing code
            from ..utils.checkpoint import read_reference_checkpoint

            ck = read_reference_checkpoint(weights)
            sd, names = ck["state_dict"], ck["names"]
        self._load_sd(sd)
        if names:
            self.model.names = names
        self.ckpt_path = str(weights) if not isinstance(weights, dict) else None
        return self

    def _load_sd(self, sd):
        sd = {k[len("model."):] if k.startswith("model.model.") else k: v for k, v in sd.items()}
        missing, unexpected = self.model.load_state_dict(sd, strict=False)
        if unexpected:
            raise KeyError(f"unexpected keys in weights: {unexpected[:5]} ...")
        # BN's num_batches_tracked counter carries no weight (the reference's checkpoints may omit it);
        # every other parameter/buffer must be present: a partial dict would leave layers at random init
        missing = [k for k in missing if not k.endswith("num_batches_tracked")]
        if missing:
            raise KeyError(f"{len(missing)} keys missing from weights: {missing[:5]} ...")
        self._sessions.clear()

    def state_dict(self):
        return self.model.state_dict()

    @property
    def names(self):
        return self.model.names

    @property
    def stride(self):
        return self.model.stride

    def fuse(self):
        self.model.fuse()
        return self

    def info(self):
        n = sum(p.numel() for p in self.model.parameters())
        return {"layers": len(self.model.model), "parameters": n}

    # ------------------------------------------------------------------ inference
    MAX_SESSIONS = 4  # a DBL-n bs32 640 fp16 session holds ~0.95 GB of HBM: keep the few most recently used

    def session(self, batch, h, w, half=False, conf=0.25, iou=0.7, max_det=300, agnostic=False, classes=None,
                multi_label=False, device=None, keep_pred=False, use_graph=True, fp8=False, clip=True,
                streams=1, gather_rows=None, nms=True, fp8_calibration=None, augment=False, embed=None, loss=None):
        """A compiled (batch, h, w, dtype, NMS settings) inference session; streams > 1 splits the batch into
        that many concurrently replayed sub-batch graphs (DetectSession); streams=None: default_streams(batch),
        the layout predict() runs and bench.py times.  augment=True: the test-time-augmentation session
        (AugmentSession: three passes, one NMS over their union; no fp8).  embed=[i, ...]: an EmbedSession -- the
        plan stops at layer max(embed) and returns the pooled layer features; the detection arguments (conf, iou, NMS
        settings) mean nothing to it and are not part of its cache key.  loss=True (or a dict of max_labels / topk /
        gains): ydbl_detect_loss behind the head on dense levels, one plan for the whole batch (DetectSession.loss,
        load_labels)."""
        loss = check_loss(loss, augment, gather_rows)
        check_segment(self.model, fp8, loss, gather_rows)  # before any device work
        check_pose(self.model, fp8, loss, gather_rows)
        if loss is not None:
            from ..nn.tasks import check_e2e_loss

            check_e2e_loss(self.model)
        embed = check_embed(embed, len(self.model.model), augment, fp8, gather_rows)
        augment = check_augment(augment, fp8, gather_rows)
        if fp8 and self.model.end2end:  # (DetectSession's guard, ahead of the device lookup)
            raise NotImplementedError("fp8=True on an end2end (YOLOv10) model: no calibration record exists for the "
                                      "YOLOv10 baseline")
        if augment and self.model.end2end:  # _predict_augment (U/nn/tasks.py:361-366): a warning and the plain pass
            from ..nn.tasks import warn_e2e_augment

            warn_e2e_augment()
            augment = False
        if augment and (self.model.segment or self.model.pose):  # the same rule: any class but DetectionModel
            from ..nn.tasks import warn_no_augment

            warn_no_augment()
            augment = False
        if loss is not None and embed is not None:
            raise ValueError("loss=True with embed: the truncated plan has no head to score")
        if streams is None:
            streams = default_streams(batch)
        dev = select_device(device)
        dtype = torch.float16 if (half or fp8) else torch.float32
        if embed is not None:
            key = ("embed", embed, batch, h, w, dtype, str(dev), use_graph, int(streams), ydbl_env())
            return self._cached_session(key, dev, lambda: EmbedSession(self.model, batch, h, w, dtype, embed, dev,
                                                                       int(streams), use_graph=use_graph))
        opt = DetectOptions(dtype, conf, iou, max_det, multi_label, agnostic, classes, clip=clip, keep_pred=keep_pred,
                            use_graph=use_graph, nms=nms, fp8=fp8, fp8_calibration=fp8_calibration, loss=loss)
        cls, rows = (AugmentSession, {}) if augment else (DetectSession, {"gather_rows": gather_rows})
        return self._cached_session(session_key(opt, batch, h, w, dev, streams, gather_rows, augment), dev,
                                    lambda: cls(self.model, batch, h, w, device=dev, streams=streams, options=opt, **rows))

    def _cached_session(self, key, dev, build):
        """The session cached under `key` (now the most recently used), else build()'s, made on `dev` in place of the
        least recently used one (its buffers go with the last reference) and stamped with the weights its plans
        folded (wsig, see _stale)."""
        s = self._sessions.get(key)
        if s is None:
            while len(self._sessions) >= self.MAX_SESSIONS:
                self._sessions.popitem(last=False)
            with torch.cuda.device(dev):
                s = build()
            s.wsig = weights_signature(self.model)
            self._sessions[key] = s
        else:
            self._sessions.move_to_end(key)
        return s

    def reset_sessions(self):
        """Drop every compiled session (after editing weights through ``.data``, which no signature sees)."""
        self._sessions.clear()
        self.model.invalidate()
        return self

    def _stale(self, s) -> bool:
        """True (and `s` dropped from the cache) when the weights changed since `s` folded them (in-place edits,
        replaced tensors: nn.tasks.weights_signature).  Called right after a launch, so the ~90 us check runs
        while the graph does."""
        if weights_signature(self.model) == s.wsig:
            return False
        for k in [k for k, v in self._sessions.items() if v is s]:
            del self._sessions[k]
        return True

    @staticmethod
    def _session_kw(args, dev, clip=True) -> dict:
        """session()'s keywords of a predict() / track() call's merged arguments; clip=False for letterboxed frames
        (the reference's NMS does not clip: boxes are clipped to the frame by scale_boxes)."""
        return dict(half=args["half"], conf=args["conf"], iou=args["iou"], max_det=args["max_det"],
                    agnostic=args["agnostic_nms"], classes=args["classes"], device=dev, fp8=args["fp8"], clip=clip,
                    streams=args["streams"], fp8_calibration=args["fp8_calibration"], augment=args["augment"])

    def _launch(self, s, shape, kw, run):
        """run(s), a launch on session `s` = self.session(*shape, **kw); when the weights were edited since `s` was
        compiled (_stale) the session is rebuilt and launched again (run(s, True)).  Returns (session, run's result)."""
        out = run(s, False)
        if self._stale(s):
            s = self.session(*shape, **kw)
            out = run(s, True)
        return s, out

    def predict(self, source=None, stream=False, **kwargs):
        """U/engine/model.py:501-560 + DetectionPredictor.postprocess (U/models/yolo/detect/predict.py:23-41).

        source (ydbl.engine.sources, after load_inference_source U/data/build.py:182-215):
          - BCHW float tensor (LoadTensor rules): run as given;
          - PIL image(s), HWC uint8 BGR ndarray frame(s), or a list of image paths (LoadPilAndNumpy): one batch;
          - str / Path: an image file, a directory, a glob or a *.txt list (LoadImagesAndVideos): batches of
            ``batch`` images (default 1) in sorted file order.
        Non-tensor sources are letterboxed to imgsz on the GPU and their boxes come back in the original
        image's coordinates.  augment=True: the reference's test-time augmentation (U/nn/tasks.py:361-398) for every
        source kind -- the (letterboxed) batch also runs at 0.83x mirrored and at 0.67x, one NMS over all three.
        """
        from .sources import check_path_source, file_batches, frames_from_images, is_frame_source

        args = {**DEFAULTS, **self.overrides, **kwargs}
        check_augment(args["augment"], args["fp8"])
        args["embed"] = check_embed(args["embed"], len(self.model.model), args["augment"], args["fp8"])
        self._check_mask_args(args)
        dev = select_device(args["device"])
        t0 = time.perf_counter()
        if source is None:
            raise ValueError("predict() needs a source (no default asset is bundled)")
        if args["embed"] is not None:
            gen = self._embed_source(source, args, dev)
            return gen if stream else list(gen)
        if not isinstance(source, torch.Tensor) and not (isinstance(source, (list, tuple)) and source
                                                         and isinstance(source[0], torch.Tensor)):
            if check_path_source(source):
                gen = (r for paths, frames in file_batches(source, args["batch"])
                       for r in self._predict_frames(frames, args, dev, time.perf_counter(), False, paths))
                return gen if stream else list(gen)
            if is_frame_source(source):
                paths, frames = frames_from_images(source)
                return self._predict_frames(frames, args, dev, t0, stream, paths)
            raise TypeError(f"unsupported source type {type(source).__name__}")
        im = check_tensor_source(source, int(self.model.stride.max()))
        if im.device != dev:  # host tensors are scaled on the host, where the reference's LoadTensor does it, then moved
            im = load_tensor_source(im).to(dev, non_blocking=True).float()
        b, _, h, w = im.shape
        kw = self._session_kw(args, dev)
        s = self.session(b, h, w, **kw)
        t1 = time.perf_counter()

        def run(s, again):
            if not again and s.can_bind(im):
                # read in place: the plans' input binding points at im, and the stem kernels apply LoadTensor's /255
                # rule from its device-side maximum (no staging copy, no host sync, no per-call copy of the outputs;
                # DetectSession.launch_bound)
                return s.launch_bound(im), None, None, None
            # LoadTensor's /255 rule on the device without a host sync: the input copy multiplies by fp32(1/255)
            # when max > 1 (torch's GPU x / 255.0 is exactly that product), by 1 otherwise
            scale = _load_tensor_scale(im)
            return (None, *s(im, scale), scale)

        s, (bo, det, cnt, scale) = self._launch(s, (b, h, w), kw, run)
        # no host sync here: each image's boxes are a view of the batch's det, cut at its count when first accessed
        # (_LazyCounts: one sync for the batch) -- on the copy path one device copy of det | count made now (the
        # session's buffers are reused by the next call); orig_img a view of the input batch (HWC, as LoadTensor
        # hands it over), made on first access.  speed["inference"] is the launch time.
        mask_of = kpt_of = None
        if self.model.pose:  # the batch's keypoints (written inside the graph): one device copy, no host sync
            kp = self._tensor_kpts(s, (h, w))
        if self.model.segment:  # one host sync for the counts, then the masks from the plan's buffers in place
            counts = cnt.tolist()
            mask_of = self._masks(s, det, counts, args, [(h, w)] * b)
            dets = det.clone()
        elif bo is not None:  # the slot's outputs, copied out of the slot on first access (or when it is reused)
            dets, counts, scale = None, _LazyCounts(lambda: bo.detach().count), (lambda: bo.detach().scale[0])
        elif getattr(s, "out_flat", None) is not None:  # det | count: one copy
            flat = s.out_flat.clone()
            dets, counts = flat[: det.numel()].view(det.shape), _LazyCounts(flat[det.numel():].view(torch.int32))
        else:
            dets, counts = det.clone(), _LazyCounts(cnt.clone())
        t2 = time.perf_counter()
        speed = {"preprocess": (t1 - t0) * 1e3 / b, "inference": (t2 - t1) * 1e3 / b, "postprocess": 0.0}
        hwc = _LazyHWC(im, scale)
        names, shape = self.model.names, (h, w)
        if bo is not None:
            box = lambda i: bo.detach().det[i, : counts[i]]  # noqa: E731
        else:
            box = lambda i: dets[i, : counts[i]]  # noqa: E731
        if self.model.pose:  # PosePredictor.postprocess (U/models/yolo/pose/predict.py:50): the boxes are rounded
            plain, box = box, (lambda i: _round_boxes(plain(i)))
            kpt_of = lambda i: kp[i, : counts[i]]  # noqa: E731
        results = [Results(lambda i=i: hwc[i], path=f"image{i}.jpg", names=names, speed=speed, orig_shape=shape,
                           boxes=lambda i=i: box(i), masks=(lambda i=i: mask_of(i)) if mask_of else None,
                           keypoints=(lambda i=i: kpt_of(i)) if kpt_of else None)
                   for i in range(b)]
        return iter(results) if stream else results

    @staticmethod
    def _tensor_kpts(s, shape):
        """A copy of the keypoints session `s` just wrote ([B, max_det, K, ndim], rows past the count zero), taken on
        the current stream before `s` can run again, after scale_coords for a tensor source (gain 1, pad 0: the clip
        to the input's extent alone, U/utils/ops.py:740-772)."""
        from ..utils.ops import clip_coords

        return clip_coords(s.kpts.clone(), shape)

    def _check_mask_args(self, args):
        """retina_masks / mask_dtype, on the host: mask_dtype must be torch.float32 (None) or torch.uint8; both mean
        nothing to a model without a Segment head and are ignored there, as the reference ignores retina_masks."""
        from ..utils.ops import mask_dtype_code

        mask_dtype_code(args["mask_dtype"])
        check_segment(self.model, args["fp8"])  # a segmentation model has no fp8 path: before the device lookup
        check_pose(self.model, args["fp8"])  # nor has a pose model

    @staticmethod
    def _masks(s, det, counts, args, shapes, boxes=None):
        """The masks of the batch session `s` just ran (SegmentationPredictor.postprocess,
        U/models/yolo/segment/predict.py:48-58), launched now on the current stream, before `s` can run again.
        counts: the host counts.  Default: process_mask(upsample=True) at the input size, one launch per sub-batch
        plan into one [sum(counts), h, w] tensor.  retina_masks: process_mask_native at each image's own shape
        (shapes[i]), one launch per image, with boxes[i] the image's kept rows already scaled to it (default: det's
        rows as they are -- a tensor source, gain 1, pad 0).  -> i -> the image's [k, H, W] masks, or None when it has
        no detection."""
        dtype = args["mask_dtype"] or torch.float32
        if not args["retina_masks"]:
            allm, offs = s.masks(counts, dtype)
            return lambda i: allm[offs[i]:offs[i + 1]] if counts[i] else None
        per = [s.masks_native(i, boxes[i] if boxes is not None else det[i, : counts[i]], shapes[i], dtype)
               if counts[i] else None for i in range(len(counts))]
        return lambda i: per[i]

    def _embed_source(self, source, args, dev):
        """predict(embed=[...]): a generator of one 1-D tensor [D] per image in source order (the predictor yields
        the embedding tensors instead of Results, U/engine/predictor.py:260-261), for every source kind predict()
        takes; on the model's device, fp16 under half=True and fp32 otherwise.  Each batch's [B, D] output is copied
        out of the session once and its rows handed over (the session's buffer is reused by the next call)."""
        from .preprocess import letterbox_batch
        from .sources import check_path_source, file_batches, frames_from_images, is_frame_source

        if not isinstance(source, torch.Tensor) and not (isinstance(source, (list, tuple)) and source
                                                         and isinstance(source[0], torch.Tensor)):
            if check_path_source(source):
                batches = (frames for _, frames in file_batches(source, args["batch"]))
            elif is_frame_source(source):
                batches = iter([frames_from_images(source)[1]])
            else:
                raise TypeError(f"unsupported source type {type(source).__name__}")
            imgsz = args["imgsz"]
            imgsz = (imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)
            stride = int(self.model.stride.max())
            for frames in batches:
                frames = [frames] if isinstance(frames, np.ndarray) and frames.ndim == 3 else list(frames)
                yield from self._embed_batch(letterbox_batch(frames, imgsz, stride=stride, device=dev), args, dev)
            return
        im = check_tensor_source(source, int(self.model.stride.max()))
        if im.device != dev:  # host tensors are scaled on the host, as in predict()
            im = load_tensor_source(im).to(dev, non_blocking=True).float()
        yield from self._embed_batch(im, args, dev, load_tensor=True)

    def _embed_batch(self, im, args, dev, load_tensor=False):
        b, _, h, w = im.shape
        kw = dict(half=args["half"], device=dev, streams=args["streams"], embed=args["embed"])
        scale = _load_tensor_scale(im) if load_tensor else None  # (as predict()'s copy path)
        _, out = self._launch(self.session(b, h, w, **kw), (b, h, w), kw, lambda s, _: s(im, scale))
        return out.clone().unbind(0)

    def embed(self, source=None, stream=False, **kwargs):
        """U/engine/model.py:467-499: image embeddings -- predict() with embed defaulting to the second-to-last
        layer (the DBL configs' last P5 FullPAD_Tunnel: 256 channels at scale n).  A list of 1-D tensors, one per
        image (a generator with stream=True)."""
        if not kwargs.get("embed"):
            kwargs["embed"] = [len(self.model.model) - 2]
        return self.predict(source, stream, **kwargs)

    def _predict_frames(self, frames, args, dev, t0, stream, paths=None):
        from .preprocess import letterbox_batch, scale_boxes

        frames = [frames] if isinstance(frames, np.ndarray) and frames.ndim == 3 else list(frames)
        imgsz = args["imgsz"]
        imgsz = (imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)
        stride = int(self.model.stride.max())
        im = letterbox_batch(frames, imgsz, stride=stride, device=dev)
        b, _, h, w = im.shape
        kw = self._session_kw(args, dev, clip=False)
        s = self.session(b, h, w, **kw)
        t1 = time.perf_counter()
        s, (det, cnt) = self._launch(s, (b, h, w), kw, lambda s, _: s(im))
        counts = cnt.tolist()
        t2 = time.perf_counter()
        scaled = []
        for i, f in enumerate(frames):
            scaled.append(scale_boxes((h, w), det[i, : counts[i]].clone(), f.shape[:2]))
        mask_of = (self._masks(s, det, counts, args, [f.shape[:2] for f in frames], scaled)
                   if self.model.segment else None)
        kpts = None
        if self.model.pose:  # PosePredictor.postprocess (U/models/yolo/pose/predict.py:49-52)
            from ..utils.ops import scale_coords

            scaled = [_round_boxes(b_) for b_ in scaled]
            kpts = [scale_coords((h, w), s.kpts[i, : counts[i]].clone(), f.shape[:2]) for i, f in enumerate(frames)]
        results = []
        for i, f in enumerate(frames):
            results.append(Results(f, path=paths[i] if paths else f"image{i}.jpg", names=self.model.names,
                                   boxes=scaled[i], masks=mask_of(i) if mask_of else None,
                                   keypoints=kpts[i] if kpts is not None else None))
        t3 = time.perf_counter()
        speed = {"preprocess": (t1 - t0) * 1e3 / b, "inference": (t2 - t1) * 1e3 / b,
                 "postprocess": (t3 - t2) * 1e3 / b}
        for r in results:
            r.speed = speed
        return iter(results) if stream else results

    __call__ = predict

    # ------------------------------------------------------------------ tracking
    def reset_trackers(self):
        """Forget every tracker's identities (the next track() call starts at id 1).  Compiled sessions stay."""
        self._trackers.clear()
        return self

    def _tracker_state(self, dev, cfg, max_det, track_rows, n, persist, max_tracks):
        from .tracker import TrackerState, settings_key

        trackers = n if track_rows == "parallel" else 1
        key = (str(dev), settings_key(cfg), int(max_det), track_rows, trackers, int(max_tracks))
        if not persist:
            self._trackers.clear()
        if track_rows == "parallel":
            other = [k for k in self._trackers if k[3] == "parallel" and k[:3] == key[:3] and k[4] != trackers]
            if other:
                raise ValueError(f"track_rows='parallel': this call has {n} rows, the trackers were started with "
                                 f"{other[0][4]}; keep the batch size, or call reset_trackers()")
        ts = self._trackers.get(key)
        if ts is None:
            with torch.cuda.device(dev):
                ts = self._trackers[key] = TrackerState(cfg, dev, max_det, trackers, max_tracks)
        return ts

    def track(self, source=None, stream=False, persist=False, tracker="bytetrack.yaml", track_rows="sequence",
              **kwargs):
        """U/engine/model.py:562-607 + U/trackers/track.py:18-87: predict() (conf defaults to 0.1, batch to 1) followed
        by ByteTrack, on the device: the association kernel (ydbl_bytetrack_update) runs behind the NMS on the same
        stream and reads its det | count where they lie.  Every source kind of predict() is accepted.  Results whose
        image got tracks carry 7-column boxes ``x1, y1, x2, y2, id, conf, cls`` (``boxes.id``, ``boxes.is_track``),
        the others keep their predicted 6 columns (``boxes.id`` None), as in the reference.

        The images of a call go through ONE tracker in row order, as consecutive frames.  persist=False resets the
        tracker before every image; persist=True keeps the identities on the model across calls (reset_trackers()
        drops them; reset_sessions() and load() do not: weights do not invalidate identities).

        tracker: ``bytetrack.yaml`` (the built-in settings), a path to a YAML of the reference's layout, or a dict.
        Unlike the reference, whose default is ``botsort.yaml``, the default here is ByteTrack, the one tracker
        implemented (``tracker_type: botsort`` raises NotImplementedError).

        track_rows="parallel" (an extension; needs persist=True and the same batch size on every call): row i of
        every call is camera i's next frame, through n independent trackers.  Ids are per tracker, each counted from
        1 (the reference's id counter is one class variable shared by all trackers).

        max_tracks (default 512): the live tracks one tracker holds; a detection that cannot start a track for lack
        of room raises RuntimeError when the batch's results are first looked at.  embed is refused (ValueError);
        fp8 and augment=True only change the detector.  For tensor sources nothing synchronises: the boxes are
        chosen (7 or 6 columns per image) on first access, with one sync for the batch."""
        from .sources import check_path_source, file_batches, frames_from_images, is_frame_source
        from .tracker import MAX_TRACKS, check_track_args, load_settings

        kwargs.setdefault("conf", 0.1)
        kwargs.setdefault("batch", 1)
        max_tracks = int(kwargs.pop("max_tracks", MAX_TRACKS))
        args = {**DEFAULTS, **self.overrides, **kwargs}
        check_track_args(args["embed"], track_rows, persist)
        cfg = load_settings(tracker)
        if max_tracks < 1:
            raise ValueError(f"max_tracks must be >= 1, got {max_tracks}")
        check_augment(args["augment"], args["fp8"])
        self._check_mask_args(args)
        if source is None:
            raise ValueError("track() needs a source (no default asset is bundled)")
        is_tensor = isinstance(source, torch.Tensor) or (isinstance(source, (list, tuple)) and source
                                                         and isinstance(source[0], torch.Tensor))
        if not is_tensor and not check_path_source(source) and not is_frame_source(source):
            raise TypeError(f"unsupported source type {type(source).__name__}")
        dev = select_device(args["device"])
        topt = (cfg, track_rows, persist, max_tracks)
        if not persist:
            self._trackers.clear()
        if is_tensor:
            res = self._track_tensor(source, args, dev, topt)
            return iter(res) if stream else res
        if check_path_source(source):
            gen = (r for paths, frames in file_batches(source, args["batch"])
                   for r in self._track_frames(frames, args, dev, topt, paths))
            return gen if stream else list(gen)
        paths, frames = frames_from_images(source)
        res = self._track_frames(frames, args, dev, topt, paths)
        return iter(res) if stream else res

    def _track_tensor(self, source, args, dev, topt):
        from .tracker import LazyTracks

        cfg, track_rows, persist, max_tracks = topt
        t0 = time.perf_counter()
        im = check_tensor_source(source, int(self.model.stride.max()))
        if im.device != dev:
            im = load_tensor_source(im).to(dev, non_blocking=True).float()
        b, _, h, w = im.shape
        kw = self._session_kw(args, dev)
        ts = self._tracker_state(dev, cfg, args["max_det"], track_rows, b, persist, max_tracks)
        s = self.session(b, h, w, **kw)
        t1 = time.perf_counter()
        scale = _load_tensor_scale(im)
        # the session's copy path; the in-place binding is not needed here
        s, (det, cnt) = self._launch(s, (b, h, w), kw, lambda s, _: s(im, scale))
        # the tracker reads the session's det | count in place, on the stream that wrote them; then one copy of them
        # for the images that keep their predicted boxes (the session's buffers are reused by the next call)
        seg, pose = self.model.segment, self.model.pose
        dets, counts = det.clone(), cnt.clone()
        if pose:  # the tracker sees the pose predictor's rounded boxes (U/models/yolo/pose/predict.py:50)
            dets[..., :4] = dets[..., :4].round()
            det = dets
        out, oc, tr, *idx = ts.update(det, cnt, [(h, w)] * b, reset_each=not persist, want_idx=seg or pose)
        lazy = LazyTracks(ts, out, oc, tr, dets, counts)
        if seg:  # the predicted masks (one sync for the counts), re-ordered like the boxes (U/trackers/track.py:83-84)
            lazy.mask_src = (self._masks(s, det, cnt.tolist(), args, [(h, w)] * b), idx[0])
        if pose:  # the keypoints follow their rows the same way; nothing synchronises
            lazy.kpt_src = (self._tensor_kpts(s, (h, w)), idx[0])
        t2 = time.perf_counter()
        speed = {"preprocess": (t1 - t0) * 1e3 / b, "inference": (t2 - t1) * 1e3 / b, "postprocess": 0.0}
        hwc = _LazyHWC(im, scale)
        names = self.model.names
        return [Results(lambda i=i: hwc[i], path=f"image{i}.jpg", names=names, speed=speed, orig_shape=(h, w),
                        boxes=lambda i=i: lazy[i], masks=(lambda i=i: lazy.masks(i)) if seg else None,
                        keypoints=(lambda i=i: lazy.keypoints(i)) if pose else None)
                for i in range(b)]

    def _track_frames(self, frames, args, dev, topt, paths=None):
        from .preprocess import letterbox_batch, scale_boxes
        from .tracker import LazyTracks

        cfg, track_rows, persist, max_tracks = topt
        t0 = time.perf_counter()
        frames = [frames] if isinstance(frames, np.ndarray) and frames.ndim == 3 else list(frames)
        imgsz = args["imgsz"]
        imgsz = (imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)
        im = letterbox_batch(frames, imgsz, stride=int(self.model.stride.max()), device=dev)
        b, _, h, w = im.shape
        kw = self._session_kw(args, dev, clip=False)
        ts = self._tracker_state(dev, cfg, args["max_det"], track_rows, b, persist, max_tracks)
        s = self.session(b, h, w, **kw)
        t1 = time.perf_counter()
        s, (det, cnt) = self._launch(s, (b, h, w), kw, lambda s, _: s(im))
        # scale_boxes to each frame's own coordinates (rows past the count scale to garbage nobody reads), then the
        # same kernel over them with the frame's shape as the clip extent
        dets, counts = det.clone(), cnt.clone()
        shapes = [tuple(f.shape[:2]) for f in frames]
        for i, shp in enumerate(shapes):
            scale_boxes((h, w), dets[i], shp)
        seg, pose = self.model.segment, self.model.pose
        if pose:  # the tracker sees the pose predictor's rounded boxes (U/models/yolo/pose/predict.py:50)
            dets[..., :4] = dets[..., :4].round()
        out, oc, tr, *idx = ts.update(dets, counts, shapes, reset_each=not persist, want_idx=seg or pose)
        lazy = LazyTracks(ts, out, oc, tr, dets, counts)
        if pose:  # scale_coords of every slot to its frame (rows past the count are never handed out)
            from ..utils.ops import scale_coords

            kp = s.kpts.clone()
            for i, shp in enumerate(shapes):
                scale_coords((h, w), kp[i], shp)
            lazy.kpt_src = (kp, idx[0])
        if seg:  # the predicted masks (one sync for the counts), re-ordered like the boxes (U/trackers/track.py:83-84)
            ch = counts.tolist()
            lazy.mask_src = (self._masks(s, det, ch, args, shapes, [dets[i, : ch[i]] for i in range(b)]), idx[0])
        t2 = time.perf_counter()
        speed = {"preprocess": (t1 - t0) * 1e3 / b, "inference": (t2 - t1) * 1e3 / b, "postprocess": 0.0}
        return [Results(f, path=paths[i] if paths else f"image{i}.jpg", names=self.model.names, speed=speed,
                        boxes=lambda i=i: lazy[i], masks=(lambda i=i: lazy.masks(i)) if seg else None,
                        keypoints=(lambda i=i: lazy.keypoints(i)) if pose else None)
                for i, f in enumerate(frames)]

    def val(self, data=None, *, coco_eval=False, loss=False, **kwargs):
        """Detection mAP (U/engine/model.py:609-643): ``data`` = a data YAML, a dataset folder, an image folder /
        list, or in-memory batches; see ydbl.engine.validator.  rect batches by default, like the reference.
        augment=True validates the test-time-augmented predictions (U/engine/validator.py: model(img, augment=...)).
        plots (default True, as in the reference's default.yaml) accumulates ``metrics.confusion_matrix`` on the
        device; False skips it.  No image files are written either way.  verbose=True prints the per-class table.
        With save_dir, dataset-backed runs write predictions.json (save_json=True) and labels/<stem>.txt
        (save_txt=True, save_conf for the confidence column); without save_dir nothing is written.
        coco_eval=True also evaluates by the COCO protocol (per-image matching on the device, ydbl_coco_match):
        ``metrics.coco_stats`` (mAP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl),
        ``metrics.coco_eval`` (COCOeval's precision / recall / scores arrays), ``validator.coco_summary()`` and, with
        save_dir, coco_stats.csv.  The Ultralytics fields keep their values.
        loss=True also scores the head's outputs against the labels (ydbl_detect_loss behind each batch's forward, on
        the letterboxed-space labels): ``metrics.val_loss`` = (box, cls, dfl) averaged over the batches
        (U/engine/validator.py:185, :205), ``val/box_loss`` / ``val/cls_loss`` / ``val/dfl_loss`` in
        ``metrics.results_dict``, ``validator.image_loss`` [images, 3] in dataset order and, with save_dir,
        val_loss.csv.  Not with augment=True (ValueError).  With the default nothing new is compiled or launched.
        A segmentation model whose batches carry ground-truth ``"masks"`` is scored on its masks too
        (ydbl.engine.validator.SegmentationValidator, U/models/yolo/segment/val.py): the result is SegmentMetrics
        (``box`` and ``seg``), ``validator.stats["tp_m"]`` the mask TP matrix.  overlap_mask=True (the default, as
        the reference's): ``"masks"`` is the uint8 index map [B, gh, gw]; False: planes [N, gh, gw] in label order.
        Without masks such a model is scored on its boxes, with a warning.
        A pose model whose batches carry ground-truth ``"keypoints"`` ([N, K, 2 or 3], in label order and in the units
        of the batch's ``bboxes``), or whose dataset's label rows have 5 + K * ndim columns, is scored on its keypoints
        too (ydbl.engine.validator.PoseValidator, U/models/yolo/pose/val.py): the result is PoseMetrics (``box`` and
        ``pose``), ``validator.stats["tp_p"]`` the keypoint TP matrix, and save_json rows gain "keypoints".  Without
        keypoints such a model is scored on its boxes, with a warning.  loss=True raises for it (v8PoseLoss)."""
        from .validator import DetectionValidator, PoseValidator, SegmentationValidator

        args = {**DEFAULTS, "conf": 0.001, "iou": 0.7, "batch": 16, "rect": True, "split": "val", "plots": True,
                "save_json": False, "save_txt": False, "save_conf": False, "save_dir": None, **kwargs,
                "coco_eval": bool(coco_eval), "loss": bool(loss)}
        check_augment(args["augment"], args["fp8"])
        check_loss(args["loss"], args["augment"], args.get("gather_rows"))
        if args["loss"]:
            from ..nn.tasks import check_e2e_loss

            check_e2e_loss(self.model)  # an end2end model's criterion is E2EDetectLoss: before any device work
        check_pose(self.model, args["fp8"], args["loss"] or None, args.get("gather_rows"))
        with_masks = with_kpts = False
        if self.model.segment:
            data, with_masks = _has_gt_masks(data, args["split"], len(self.model.names))
            if not with_masks:
                _warn_seg_val()
            elif args.get("gather_rows") is not None:
                raise ValueError("mask metrics are not implemented for the batch-sharded predictor (gather_rows)")
        if self.model.pose:
            data, with_kpts = _has_gt_masks(data, args["split"], len(self.model.names), key="keypoints",
                                            kpt_shape=self.model.kpt_shape)
            if not with_kpts:
                _warn_pose_val()
        # kept: its per-image stats (tp, conf, pred_cls, target_cls; tp_m with mask metrics, tp_p with keypoints)
        cls = SegmentationValidator if with_masks else PoseValidator if with_kpts else DetectionValidator
        self.validator = cls(self, args)
        return self.validator(data)


def _round_boxes(boxes):
    """A copy of the rows with the box columns rounded: scale_boxes(...).round() of PosePredictor.postprocess
    (U/models/yolo/pose/predict.py:50)."""
    boxes = boxes.clone()
    boxes[:, :4] = boxes[:, :4].round()
    return boxes


def _has_gt_masks(data, split="val", n_names=0, key="masks", kpt_shape=None):
    """(data, whether val() computes mask metrics on it): an iterable of in-memory batches does when its first batch
    carries "masks" (the iterable is handed back with that batch in place); a dataset does when at least one label
    file of the split holds a polygon row.  key="keypoints" with kpt_shape: the same question for a pose model's
    keypoint metrics (a dataset does when a label row has 5 + K * ndim columns)."""
    import itertools
    import os

    if data is None:
        return data, False
    if isinstance(data, (str, os.PathLike, dict)):
        from .dataset import split_has_keypoints, split_has_segments
        from .validator import val_source

        src = val_source(data, split, n_names)[0]
        return data, split_has_keypoints(src, kpt_shape) if key == "keypoints" else split_has_segments(src)
    if isinstance(data, (list, tuple)):  # known up front: said before any device work
        has = [isinstance(b, dict) and key in b for b in data]
        if any(has) and not all(has):
            raise ValueError(f"val(): only some batches carry '{key}'; {key[:-1]} metrics need them in every batch")
    it = iter(data)
    first = next(it, None)
    if first is None:
        return [], False
    return itertools.chain([first], it), isinstance(first, dict) and key in first


_SEG_VAL_WARNED = False


def _warn_seg_val():
    """val() on a segmentation model: the box report, as for Detect; the mask metrics (SegmentationValidator,
    SegmentMetrics) are not computed.  Said once."""
    global _SEG_VAL_WARNED
    if not _SEG_VAL_WARNED:
        import warnings

        warnings.warn("val() on a segmentation model reports the box metrics only: mask metrics (mask mAP) are not "
                      "computed", stacklevel=3)
        _SEG_VAL_WARNED = True


_POSE_VAL_WARNED = False


def _warn_pose_val():
    """val() on a pose model without ground-truth keypoints: the box report, as for Detect.  Said once."""
    global _POSE_VAL_WARNED
    if not _POSE_VAL_WARNED:
        import warnings

        warnings.warn("val() on a pose model without ground-truth keypoints reports the box metrics only: keypoint "
                      "metrics (pose mAP) are not computed", stacklevel=3)
        _POSE_VAL_WARNED = True


class YOLO(Model):
    """U/models/yolo/model.py:52-100 — detect task only."""

    @property
    def task_map(self):
        return {"detect": {"model": DetectionModel, "predictor": DetectSession}}
