"""Model construction (YAML -> layers) and plan compilation for the MI355X path.

Construction follows U/nn/tasks.py:947-1242 (parse_model, yaml_model_load,
guess_model_scale) for the layer types the DBL configurations use; modules
are looked up BY CLASS NAME, exactly like the reference's plugin mechanism
(``globals()[m]``, U/nn/tasks.py:974), so ``register_module`` can swap in
another implementation with the same constructor signature.

``DetectionModel.compile(batch, h, w, dtype)`` turns the layer list into a
``Plan`` (U/nn/tasks.py:145-172 ``_predict_once`` order), with every Concat
input written in place into its slice of the concat buffer.
"""

from __future__ import annotations

import ast
import contextlib
import json
import math
import operator
import os
import re
from copy import deepcopy
from pathlib import Path

import torch
import torch.nn as nn

from ..runtime import TV, Plan, round_up, weights_signature, ydbl_env  # noqa: F401 (re-exported)
from .. import _lib
from . import modules as M

CFG_DIR = Path(__file__).resolve().parent.parent / "cfg" / "models"

# class-name registry = the reference's globals() lookup
REGISTRY: dict[str, type] = {
    c.__name__: c
    for c in (M.Conv, M.DWConv, M.DSConv, M.GhostConv, M.Concat, M.Bottleneck, M.C2f, M.C3, M.C3Ghost,
              M.GhostBottleneck, M.DSBottleneck, M.DSC3k, M.DSC3k2, M.HyperACE, M.DownsampleConv,
              M.FullPAD_Tunnel, M.DySample, M.LSKblock, M.Detect, M.AAttn, M.ABlock, M.A2C2f, M.SPPF, M.C3k, M.C3k2,
              M.Attention, M.PSABlock, M.C2PSA, M.PSA, M.SCDown, M.RepVGGDW, M.CIB, M.C2fCIB, M.v10Detect, M.Proto,
              M.Segment, M.Pose)
}
REGISTRY["nn.Upsample"] = M.Upsample  # the one torch.nn layer name the v13 YAMLs use (U/nn/tasks.py:972-973)
_C1C2 = {"Conv", "DWConv", "GhostConv", "Bottleneck", "GhostBottleneck", "C2f", "C3", "C3Ghost", "DSC3k2", "DSConv",
         "DSBottleneck", "A2C2f", "SPPF", "C3k2", "C2PSA", "PSA", "SCDown", "C2fCIB"}
_REPEAT_ARG = {"C2f", "C3", "C3Ghost", "DSC3k2", "A2C2f", "C3k2", "C2PSA", "C2fCIB"}
_DETECT = {"Detect", "v10Detect", "Segment", "Pose"}  # U/nn/tasks.py:1107-1112
_C1_ONLY = {"DySample", "LSKblock"}


def register_module(cls, name: str | None = None):
    """Plug a module class in under a YAML name (same constructor contract as the reference, whose parse_model
    resolves names through globals(), U/nn/tasks.py:974).  Either contract works: a class with
    ``emit(plan, x, out)`` (HIP launches, as the built-ins) or a plain torch ``forward(x)``, which runs inside the
    compiled plan as a captured torch step on NCHW views of its inputs (nn.modules.emit_torch).  Channel
    bookkeeping for a plugin name follows the reference's rule for names it does not know (c2 = ch[f])."""
    REGISTRY[name or cls.__name__] = cls
    return cls


def normalize_embed(embed, n_layers: int) -> tuple:
    """The layer indices of ``embed=`` as _predict_once uses them (U/nn/tasks.py:158-171): ascending and each once,
    whatever the order of the list (the segments are appended in layer order and the forward returns at max(embed)).
    Valid: integers in [0, n_layers - 2] -- every layer but the head, whose output is no feature map; the reference
    never returns (index past the model) or fails inside the pool (the head) for the others.  Pure host arithmetic:
    callers run it before anything is compiled or a device is touched."""
    if isinstance(embed, (int, float)) and not isinstance(embed, bool):
        embed = [embed]
    try:
        items = list(embed)
    except TypeError:
        raise ValueError(f"embed={embed!r}: a list of layer indices expected") from None
    if not items:
        raise ValueError("embed: an empty list names no layer")
    out = set()
    for i in items:
        try:
            if isinstance(i, bool):
                raise TypeError
            i = operator.index(i)
        except TypeError:
            raise ValueError(f"embed index {i!r} is not an integer (valid layers: 0..{n_layers - 2})") from None
        if not 0 <= i <= n_layers - 2:
            raise ValueError(f"embed index {i} is outside the valid layer range 0..{n_layers - 2} "
                             f"(layer {n_layers - 1} is the detection head)")
        out.add(i)
    return tuple(sorted(out))


def make_divisible(x, divisor):
    """U/utils/ops.py:130-143."""
    if isinstance(divisor, torch.Tensor):
        divisor = int(divisor.max())
    return math.ceil(x / divisor) * divisor


def guess_model_scale(model_path) -> str:
    """U/nn/tasks.py:1227-1242."""
    m = re.search(r"yolo[v]?\d+([nslmx])", Path(model_path).stem)
    return m.group(1) if m else ""


def yaml_model_load(path) -> dict:
    """U/nn/tasks.py:1211-1224: 'yolov13n_DBL.yaml' -> unified 'yolov13_DBL' config with scale 'n'.

    Built-in configs live in ydbl/cfg/models/*.json; an existing .yaml/.json path is read directly, and a scaled
    name that does not exist beside an existing unified file ('yolov13n.yaml' next to 'yolov13.yaml') reads that.
    """
    path = Path(path)
    unified = re.sub(r"(\d+)([nslmx])(.+)?$", r"\1\3", path.stem)
    src = path
    if not path.exists() and (path.parent / f"{unified}{path.suffix}").exists():
        # 'yolov13n.yaml' next to a 'yolov13.yaml': the unified file at the scale of the name (U/nn/tasks.py:1216-1219)
        src = path.parent / f"{unified}{path.suffix}"
    if src.exists():
        if src.suffix in (".yaml", ".yml"):
            import yaml

            d = yaml.safe_load(src.read_text())
        else:
            d = json.loads(src.read_text())
    else:
        for cand in (CFG_DIR / f"{unified}.json", CFG_DIR / f"{path.stem}.json"):
            if cand.exists():
                d = json.loads(cand.read_text())
                break
        else:
            raise FileNotFoundError(f"model config '{path}' not found (built-in: {sorted(p.stem for p in CFG_DIR.glob('*.json'))})")
    d["scale"] = guess_model_scale(path)
    d["yaml_file"] = str(path)
    return d


def parse_model(d: dict, ch: int = 3, verbose: bool = False):
    """U/nn/tasks.py:947-1208 for the module set of the DBL configs."""
    legacy = True
    nc, scales = d.get("nc"), d.get("scales")
    depth, width, max_channels = d.get("depth_multiple", 1.0), d.get("width_multiple", 1.0), float("inf")
    scale = "?"
    if scales:
        scale = d.get("scale") or tuple(scales.keys())[0]
        if scale not in scales:
            raise KeyError(f"scale '{scale}' not defined by this config (available: {list(scales)})")
        depth, width, max_channels = scales[scale]
    ch = [ch]
    layers, save, c2 = [], [], ch[-1]
    for i, (f, n, name, args) in enumerate(d["backbone"] + d["head"]):
        if name not in REGISTRY:
            raise KeyError(f"module '{name}' (layer {i}) has no MI355X implementation")
        m = REGISTRY[name]
        args = [nc if a == "nc" else d.get("kpt_shape") if a == "kpt_shape" else a for a in args]
        for j, a in enumerate(args):  # YAML delivers 'None' as a string (U/nn/tasks.py:1000-1003)
            if isinstance(a, str):
                with contextlib.suppress(ValueError, SyntaxError):
                    args[j] = ast.literal_eval(a)
        n = n_ = max(round(n * depth), 1) if n > 1 else n
        if name in _C1C2:
            c1, c2 = ch[f], args[0]
            if c2 != nc:
                c2 = make_divisible(min(c2, max_channels) * width, 8)
            args = [c1, c2, *args[1:]]
            if name in _REPEAT_ARG:
                args.insert(2, n)
                n = 1
            if name in ("DSC3k2", "C3k2"):  # U/nn/tasks.py:1084-1085
                legacy = False
            if name == "A2C2f":  # U/nn/tasks.py:1087-1091
                legacy = False
                if scale in "lx":
                    args += [True, 1.5]
        elif name == "Concat":
            c2 = sum(ch[x] for x in f)
        elif name in _DETECT:
            args.append([ch[x] for x in f])
            if name == "Segment":  # U/nn/tasks.py:1109-1110: the proto width scales like a channel count
                args[2] = make_divisible(min(args[2], max_channels) * width, 8)
        elif name == "HyperACE":
            legacy = False
            c1 = ch[f[1]]
            c2 = make_divisible(min(args[0], max_channels) * width, 8)
            he = args[1]
            if scale in "n":
                he = int(args[1] * 0.5)
            elif scale in "x":
                he = int(args[1] * 1.5)
            args = [c1, c2, n, he, *args[2:]]
            n = 1
        elif name == "DownsampleConv":
            c1 = ch[f]
            c2 = c1 * 2
            args = [c1]
        elif name == "FullPAD_Tunnel":
            c2 = ch[f[0]]
        elif name in _C1_ONLY:
            c1 = c2 = ch[f]
            args = [c1, *args[1:]]
        else:
            c2 = ch[f]
        if name in ("Detect", "Segment", "Pose"):
            m.legacy = legacy  # class attribute, as the reference sets it (U/nn/tasks.py:1111-1112)
            m_ = m(*args)
            m_.legacy = legacy  # and on the instance: a yolov8 (legacy) and a yolo11 model may live in one process
        elif name == "v10Detect":  # builds its own class branch: Detect's class attribute is left as it is
            m_ = m(*args)
        else:
            m_ = nn.Sequential(*(m(*args) for _ in range(n))) if n > 1 else m(*args)
        m_.np = sum(x.numel() for x in m_.parameters())
        m_.i, m_.f, m_.type = i, f, name
        if verbose:
            print(f"{i:>3}{str(f):>20}{n_:>3}{m_.np:10.0f}  {name:<20}{str(args):<30}")
        save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
        layers.append(m_)
        if i == 0:
            ch = []
        ch.append(c2)
    return nn.Sequential(*layers), sorted(save)


class DetectionModel(nn.Module):
    """U/nn/tasks.py:313-359 + BaseModel.fuse (:207-235)."""

    def __init__(self, cfg="yolov13n_DBL.yaml", ch=3, nc=None, verbose=False, data_kpt_shape=(None, None)):
        super().__init__()
        self.yaml = cfg if isinstance(cfg, dict) else yaml_model_load(cfg)
        ch = self.yaml["ch"] = self.yaml.get("ch", ch)
        if nc and nc != self.yaml["nc"]:
            self.yaml["nc"] = nc
        # PoseModel.__init__ (U/nn/tasks.py): the dataset's kpt_shape overrides the config's
        if data_kpt_shape is not None and any(data_kpt_shape) and "kpt_shape" in self.yaml \
                and list(data_kpt_shape) != list(self.yaml["kpt_shape"]):
            self.yaml["kpt_shape"] = list(data_kpt_shape)
        self.model, self.save = parse_model(deepcopy(self.yaml), ch=ch, verbose=verbose)
        self.names = {i: f"{i}" for i in range(self.yaml["nc"])}
        self.inplace = self.yaml.get("inplace", True)
        m = self.model[-1]
        self.end2end = bool(getattr(m, "end2end", False))  # U/nn/tasks.py:331
        self.segment = isinstance(m, M.Segment)  # SegmentationModel (U/nn/tasks.py:439-452): the same forward
        self.pose = isinstance(m, M.Pose)  # PoseModel: the same forward, the head also returns the keypoints
        if self.pose:
            self.kpt_shape = list(m.kpt_shape)
        # Stride probe by shape propagation at 256x256 (the reference runs a train-mode forward on
        # zeros, U/nn/tasks.py:337-350; only its output shapes are used for the strides).
        s = 256
        levels = self.compile(1, s, s, torch.float32, device="meta").levels
        m.stride = torch.tensor([s / lv.h for lv in levels])
        self.stride = m.stride
        m.bias_init()
        for mod in self.modules():  # U/utils/torch_utils.py:410-420
            if isinstance(mod, nn.BatchNorm2d):
                mod.eps = 1e-3
                mod.momentum = 0.03
        self._fused = False

    @property
    def nc(self):
        return self.model[-1].nc

    MAX_FORWARD_SESSIONS = 2

    def forward(self, x, *args, **kwargs):
        """BaseModel.forward -> predict -> _predict_once (U/nn/tasks.py:109-172) with Detect's inference return
        (U/nn/modules/head.py:108-118): ``(y, feats)``, y [B, 4+nc, A] = decoded xywh boxes (pixels) + class
        scores (Detect._inference, head.py:143-181), feats = the per-level head maps cat(box, cls)
        [B, 64+nc, H_i, W_i].  This is the call AutoBackend makes (U/nn/autobackend.py:503-528, ``self.model(im)``).

        Runs the compiled HIP plan of x's (batch, h, w, dtype) on x's device -- forward + decode, no NMS --
        replayed as a hipGraph; fp16 input takes the half path (AutoBackend fp16, autobackend.py:145-155).
        BN is folded and the semantics are always inference (eval) ones; profile / visualize are not on this path,
        and neither is training: a dict input returns ``self.loss(x)``, the forward-only detection loss.  embed=[i, ...]: _predict_once's early return (U/nn/tasks.py:158-171)
        -- the tuple of B row tensors [sum C_i] in x's dtype, the named layers' pooled outputs in ascending layer
        order, from a plan that stops at max(embed) (engine.session.EmbedSession).  augment=True: _predict_augment (U/nn/tasks.py:361-398) --
        returns ``(y, None)``, y [B, 4+nc, A_tot] the three passes' de-scaled, de-flipped, tail-clipped predictions
        side by side (engine.session.AugmentSession).  Returns fresh tensors (the plan's buffers are reused by the
        next call).  CPU tensors raise: there is no CPU execution path."""
        if isinstance(x, dict):  # BaseModel.forward (U/nn/tasks.py:109-112): a batch dict asks for the loss
            return self.loss(x, *args, **kwargs)
        if args or any(kwargs.get(k) for k in ("profile", "visualize")):
            raise NotImplementedError("profile / visualize are outside the inference path")
        augment = bool(kwargs.get("augment"))
        embed = kwargs.get("embed")
        if embed:  # checked before any device work
            if augment:
                raise ValueError("embed with augment=True: the augmented forward has no embedding (the reference "
                                 "silently ignores embed there)")
            embed = normalize_embed(embed, len(self.model))
        if not isinstance(x, torch.Tensor) or x.ndim != 4:
            raise TypeError("DetectionModel.forward takes a BCHW tensor")
        if x.device.type != "cuda":
            raise RuntimeError(f"ydbl runs on MI355X (gfx950) only: input on {x.device}, move it to a cuda device")
        if x.dtype not in (torch.float32, torch.float16):
            raise TypeError(f"input dtype {x.dtype}: float32 or float16 (half) expected")
        if x.shape[1] != self.yaml["ch"]:
            raise ValueError(f"input has {x.shape[1]} channels, the model {self.yaml['ch']}")
        if embed:  # _predict_once's early return (U/nn/tasks.py:168-171): torch.unbind(torch.cat(embeddings, 1), 0)
            return self._run(x, embed=embed)[1].to(x.dtype, copy=True).unbind(0)
        if self.end2end:
            # an end2end head (v10Detect.forward_end2end, U/nn/modules/head.py:120-141): (y [B, min(300, A), 6],
            # {"one2many", "one2one"}) from the head's own forward on the neck's maps -- Detect.postprocess as a top-k
            # with no threshold and no clipping.  _predict_augment (U/nn/tasks.py:361-366) warns and runs this pass
            if augment:
                warn_e2e_augment()
            return self._run(x, e2e=True)[1]
        if (self.segment or self.pose) and augment:  # _predict_augment (U/nn/tasks.py:361-366): any class but DetectionModel
            warn_no_augment()
            augment = False
        s, _ = self._run(x, augment=augment)
        y = s.pred.to(x.dtype, copy=True)
        if augment:
            return y, None
        feats = [f.contiguous() for f in s.feats()]
        if self.segment:  # Segment.forward (U/nn/modules/head.py:259-271): (cat([y, mc], 1), (feats, mc, p))
            mc, p = s.seg_outputs()
            return torch.cat([y, mc], 1), (feats, mc, p)
        if self.pose:  # Pose.forward (U/nn/modules/head.py:364-372): (cat([y, pred_kpt], 1), (feats, kpt))
            kpt = s.pose_outputs()
            views = s.parts[0].compiled.plan.pose
            return torch.cat([y, M.kpts_decode(kpt, views, self.stride.tolist(), self.kpt_shape[1])], 1), (feats, kpt)
        return y, feats

    MAX_LABELS = 300  # per image: the capacity of the in-graph loss's label buffer (loss(batch) with preds=None)

    def init_criterion(self):
        """U/nn/tasks.py:358-359 (DetectionModel.init_criterion)."""
        from ..utils.loss import v8DetectionLoss

        check_e2e_loss(self)
        return v8DetectionLoss(self, max_labels=self.MAX_LABELS)

    def loss(self, batch, preds=None):
        """BaseModel.loss (U/nn/tasks.py:294-306): ``(loss.sum() * batch_size, loss_items)`` of a batch dict
        ``{"img", "batch_idx", "cls", "bboxes"}`` (bboxes: normalised xywh of img), fp32 device tensors, forward only.
        preds=None: the forward and the loss are ONE captured graph -- a session whose Detect levels stay dense with
        ydbl_detect_loss behind the head, reading them in place; the labels go through a fixed-capacity buffer
        (MAX_LABELS per image) refilled before the replay, like the input.  An image with more labels, or a class
        outside [0, nc), raises ValueError on the host before anything is launched.  preds given (the ``feats`` list
        or the ``(y, feats)`` tuple of forward): the criterion alone (utils.loss.v8DetectionLoss)."""
        check_e2e_loss(self)
        if getattr(self, "criterion", None) is None:
            self.criterion = self.init_criterion()
        if preds is not None:
            return self.criterion(preds, batch)
        x = batch["img"]
        if not isinstance(x, torch.Tensor) or x.ndim != 4:
            raise TypeError("DetectionModel.loss takes batch['img'] as a BCHW tensor")
        b, _, h, w = x.shape
        gt = self.criterion.preprocess(batch, b, (h, w))  # host guards: before any device work
        if x.device.type != "cuda":
            raise RuntimeError(f"ydbl runs on MI355X (gfx950) only: input on {x.device}, move it to a cuda device")
        if x.dtype not in (torch.float32, torch.float16):
            raise TypeError(f"input dtype {x.dtype}: float32 or float16 (half) expected")
        if x.shape[1] != self.yaml["ch"]:
            raise ValueError(f"input has {x.shape[1]} channels, the model {self.yaml['ch']}")
        s, _ = self._run(x, gt, loss=True)
        items = s.loss.loss.clone()
        return items.sum() * b, items

    def _run(self, x, labels=None, **kw):
        """One launch of x -- `labels` refilled into a loss session's buffer first -- on the compiled session of its
        shape and dtype (_forward_session(**kw)).  The weights' signature is checked while the graph runs; when they
        were edited since the plan was compiled, the session is rebuilt and run again.  Returns (session, outputs)."""
        b, _, h, w = x.shape
        fresh = None
        for _ in range(2):
            s = self._forward_session(b, h, w, x.dtype == torch.float16, x.device, fresh=fresh, **kw)
            if labels is not None:
                s.load_labels(labels)
            out = s(x.float())
            fresh = weights_signature(self)
            if fresh == s.wsig:
                break
        return s, out

    def _forward_session(self, b, h, w, half, device, fresh=None, augment=False, embed=None, loss=False, e2e=False):
        from ..engine.session import (AugmentSession, DetectOptions, DetectSession, E2EForwardSession, EmbedSession,
                                      default_streams)

        cache = self.__dict__.setdefault("_fwd_sessions", {})
        # compiled plans hold the routing of the YDBL_* switches at build time (part of the key) and BN-folded
        # copies of the weights (the session's wsig, checked by forward() after each launch)
        key = ((b, h, w, half, str(device), ydbl_env(), augment) + ((embed,) if embed else ())
               + ((("loss", self.MAX_LABELS),) if loss else ()) + (("e2e",) if e2e else ()))
        s = cache.pop(key, None)
        if s is not None and fresh is not None and s.wsig != fresh:
            s = None  # weights changed since this plan was built
        if s is None:
            while len(cache) >= self.MAX_FORWARD_SESSIONS:
                cache.pop(next(iter(cache)))
            dtype = torch.float16 if half else torch.float32
            with torch.cuda.device(device):
                if embed:
                    s = EmbedSession(self, b, h, w, dtype, embed, device=device, streams=default_streams(b))
                elif e2e:
                    s = E2EForwardSession(self, b, h, w, dtype, device=device)
                else:  # forward + decode, no NMS; loss: + ydbl_detect_loss on dense levels, one plan (a loss session
                    # never splits: one normaliser for the batch)
                    opt = DetectOptions(dtype, keep_pred=True, nms=False,
                                        loss={"max_labels": self.MAX_LABELS} if loss else None)
                    s = (AugmentSession if augment else DetectSession)(self, b, h, w, device=device,
                                                                       streams=default_streams(b), options=opt)
            s.wsig = weights_signature(self)
        cache[key] = s  # most recently used last
        return s

    def invalidate(self):
        """Drop every compiled forward plan (after editing weights through ``.data``)."""
        self.__dict__.pop("_fwd_sessions", None)
        return self

    def load_state_dict(self, *args, **kwargs):
        """nn.Module.load_state_dict; compiled forward plans hold folded copies of the weights, so they go."""
        self.invalidate()
        return super().load_state_dict(*args, **kwargs)

    def fuse(self, verbose=False):
        """BaseModel.fuse (U/nn/tasks.py:207-235).  Conv's BN folding happens when a plan is compiled (exactly
        fuse_conv_and_bn's arithmetic); a RepVGGDW is folded here as the reference folds it (block.py:791-815: both
        branches' BN, the 3x3 padded into the 7x7, one nn.Conv2d left), which the plan then takes as it is."""
        for m in self.modules():
            if isinstance(m, M.RepVGGDW):
                m.fuse()
        self.invalidate()
        self._fused = True
        return self

    def is_fused(self):
        return self._fused

    def compile(self, batch: int, h: int, w: int, dtype=torch.float16, device="cuda", bind=None, embed=None,
                embed_out=None, head_forward=False) -> "CompiledModel":
        """Build the launch plan of one forward: input NCHW fp32 [batch,3,h,w] -> per-level head outputs.
        The plan reads its batch through an input binding (include/ydbl.h ydbl_input_bind): bind_ptr, a device int64
        holding the batch pointer (initially the plan's own staging buffer ``input``), and bind_amax, a device fp32
        batch maximum for LoadTensor's /255 rule (0: scale 1).  bind = (bind_ptr, bind_amax) shares them with a
        caller (a split session: one word per sub-batch plan, one maximum).

        embed = layer indices (normalize_embed): the truncated plan of _predict_once's early return
        (U/nn/tasks.py:158-171).  Layers 0..max(embed) only -- no head, no concat buffer past the cut (a producer whose
        concat lies past it writes a buffer of its own) -- and right behind the launches of each named layer one
        ydbl_global_avgpool ("embed.pool") of its output into its columns of ``embed_out`` [batch, sum C_i] (plan
        dtype; a caller's 2-D view with its own row stride for a split session).  The result has levels = None.

        head_forward (an end2end head): the head's whole inference forward (v10Detect._forward_plan: both branch sets,
        decode, top-k) in place of its emit; the result has levels = None and ``finish`` = the call that returns the
        forward's outputs as fresh tensors."""
        plan = Plan(torch.device(device), dtype)
        if embed is not None:
            embed = normalize_embed(embed, len(self.model))
        inp = plan.alloc(batch, h, w, 8)  # RGB padded to 8 channels (16-byte vectors)
        x_nchw = torch.empty((batch, self.yaml["ch"], h, w), dtype=torch.float32, device=plan.device)
        plan.buffers.append(x_nchw)
        if bind is None:
            bind = (torch.empty(1, dtype=torch.int64, device=plan.device),
                    torch.zeros(1, dtype=torch.float32, device=plan.device))
        bind_ptr, bind_amax = bind
        bind_ptr.fill_(x_nchw.data_ptr())
        plan.buffers += [bind_ptr, bind_amax]
        ib = _lib.InputBind(bind_ptr.data_ptr(), bind_amax.data_ptr())
        # Concat outputs are allocated up front; their producers write straight into the slices.
        layers = list(self.model)
        if embed is not None:
            layers = layers[: embed[-1] + 1]  # nothing past the cut is shaped, allocated or emitted
        shapes = _propagate_shapes(layers, batch, h, w, self.yaml["ch"])
        pool = None
        if embed is not None:
            widths = [shapes[i][3] for i in embed]
            if embed_out is None:
                embed_out = torch.empty((batch, sum(widths)), dtype=dtype, device=plan.device)
            if (tuple(embed_out.shape) != (batch, sum(widths)) or embed_out.dtype != dtype
                    or embed_out.stride(1) != 1 or embed_out.device.type != plan.device.type):
                raise ValueError(f"embed_out: a [{batch}, {sum(widths)}] {dtype} view with unit column stride "
                                 f"on {plan.device} expected")
            plan.buffers.append(embed_out)
            col = dict(zip(embed, [sum(widths[:k]) for k in range(len(widths))]))
            views = {}

            def pool(i, v):
                """Layer i's output view v -> its columns of embed_out (emitted right behind the layer's launches:
                no later in-place consumer of v can come between them)."""
                if i not in col:
                    return
                d = _lib.AvgPoolDesc(v.struct(), embed_out.data_ptr() + col[i] * embed_out.element_size(),
                                     embed_out.stride(0), None, 0)
                need = int(_lib.lib.ydbl_global_avgpool_workspace(d))
                if need < 0:
                    _lib.check(1, "ydbl_global_avgpool_workspace")
                ws = plan.scratch(need) if need else None
                if ws is not None:
                    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
                plan.launch("ydbl_global_avgpool", d, what="embed.pool", keep=[d, v])
                views[i] = v
        out_hint: dict[int, TV] = {}
        cat_buf: dict[int, TV] = {}
        for m in layers:
            if m.type == "Concat":
                srcs = [m.i - 1 if j == -1 else j for j in m.f]
                n_, h_, w_, _ = shapes[srcs[0]]
                buf = plan.alloc(n_, h_, w_, sum(shapes[j][3] for j in srcs))
                cat_buf[m.i] = buf
                off = 0
                for j in srcs:
                    c = shapes[j][3]
                    if j not in out_hint and layers[j].type not in ("Concat",):
                        out_hint[j] = buf.cslice(off, c)
                    off += c
        y: list[TV | None] = []
        x = inp
        stem = layers[0] if M.stem_ok(layers[0], self.yaml["ch"]) and 0 not in out_hint else None
        # layers 0+1 as one kernel when layer 0's map feeds layer 1 only (the full-resolution map never
        # reaches HBM); YDBL_NO_STEM2=1 keeps them separate (A/B switch)
        used_later = any(j == 0 for m in layers[2:] for j in ([m.f] if isinstance(m.f, int) else m.f))
        used_later = used_later or (embed is not None and 0 in embed)  # layer 0's map is pooled: it must exist
        stem2 = (stem is not None and len(layers) > 1 and not used_later and not os.environ.get("YDBL_NO_STEM2")
                 and M.stem2_ok(layers[0], layers[1], self.yaml["ch"], dtype))
        if stem is None:
            plan.launch("ydbl_input_nchw_to_nhwc", x_nchw.data_ptr(), batch, self.yaml["ch"], h, w, 1.0, inp.struct(),
                        ib, what="input", keep=[ib])
        for m in layers:
            plan.cur_layer = m.i  # (ydbl.quant names fp8 candidates by the layer that emitted them)
            if stem2 and m is layers[1]:
                y.append(x)
            elif m is stem and stem2:  # preprocess + layers 0 and 1 in one kernel
                x = M.emit_stem2(layers[0], layers[1], plan, x_nchw, batch, self.yaml["ch"], h, w,
                                 cat_buf.get(1, out_hint.get(1)), bind=ib)
                y.append(None)  # layer 0's map is never materialised
                continue
            elif m is stem:  # preprocess + first Conv fused, straight from the NCHW batch
                x = M.emit_stem(m, plan, x_nchw, batch, self.yaml["ch"], h, w, bind=ib)
                y.append(x)
            else:
                if m.f != -1:
                    x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
                out = cat_buf.get(m.i, out_hint.get(m.i))
                if head_forward and m is layers[-1]:
                    finish, x = m._forward_plan(plan, x), None
                else:
                    x = M.emit_module(m, plan, x, out)
                y.append(x)
            if pool is not None:
                pool(m.i, x)
        cm = CompiledModel(plan, x_nchw, inp, x if embed is None else None, self.model[-1])
        if embed is not None:
            cm.embed, cm.embed_out, cm.embed_views = embed, embed_out, views
        if head_forward:
            cm.finish = finish
        cm.bind_ptr, cm.bind_amax = bind_ptr, bind_amax
        # the InputBind records the launches read (retargeted by CompiledModel.set_bind)
        cm.bind_holders = [st.args[0].bind if st.fn.__name__ == "ydbl_conv_stem2" else st.args[-1]
                           for st in plan.steps if st.fn.__name__ in ("ydbl_conv_stem2", "ydbl_conv_stem",
                                                                       "ydbl_input_nchw_to_nhwc")]
        cm.set_bind(None)  # the plan's own staging buffer, read directly (DetectSession slot 0)
        return cm


_E2E_AUGMENT_WARNED = False


def warn_e2e_augment():
    """_predict_augment on an end2end model (U/nn/tasks.py:361-366): a warning, once, and the plain pass."""
    global _E2E_AUGMENT_WARNED
    if not _E2E_AUGMENT_WARNED:
        import warnings

        warnings.warn("End2End model does not support 'augment=True' prediction. Reverting to single-scale "
                      "prediction.", stacklevel=3)
        _E2E_AUGMENT_WARNED = True


def warn_no_augment():
    """_predict_augment on a model that is not a plain DetectionModel (U/nn/tasks.py:361-366; a segmentation model):
    a warning, once, and the plain pass."""
    global _SEG_AUGMENT_WARNED
    if not _SEG_AUGMENT_WARNED:
        import warnings

        warnings.warn("Model does not support 'augment=True', reverting to single-scale prediction.", stacklevel=3)
        _SEG_AUGMENT_WARNED = True


_SEG_AUGMENT_WARNED = False


def check_e2e_loss(model):
    """The criterion of an end2end model is E2EDetectLoss (U/utils/loss.py:728-743), the dual-assignment loss over
    both branch sets: not implemented.  Nor is a segmentation model's (v8SegmentationLoss).  Raised on the host, before
    any device work."""
    if getattr(model, "segment", False):
        raise NotImplementedError("the loss of a segmentation model is v8SegmentationLoss, which is not implemented")
    if getattr(model, "pose", False):
        raise NotImplementedError("the loss of a pose model is v8PoseLoss, which is not implemented")
    if getattr(model, "end2end", False):
        raise NotImplementedError("the loss of an end2end (YOLOv10) model is E2EDetectLoss (one2many + one2one "
                                  "assignment), which is not implemented")


class CompiledModel:
    """A compiled forward: ``input`` (NCHW fp32 staging buffer) -> ``levels`` (per-level NHWC head outputs);
    bind_ptr / bind_amax: its input binding (DetectionModel.compile).  A plan compiled with embed= stops at the last
    named layer: ``levels`` is None, ``embed`` the normalised indices, ``embed_out`` the [batch, D] pooled features
    and ``embed_views`` {layer: the output view its pool reads}."""

    embed = embed_out = embed_views = None

    def __init__(self, plan: Plan, x_nchw: torch.Tensor, inp: TV, levels: list[TV] | None, detect: M.Detect):
        self.plan, self.input, self.inp, self.levels, self.detect = plan, x_nchw, inp, levels, detect

    def feats(self):
        """Reference-layout per-level outputs x[i] = cat(box, cls) as NCHW views (no copy)."""
        return [lv.nchw() for lv in self.levels]

    def set_bind(self, ptr: torch.Tensor | None, amax: torch.Tensor | None = None):
        """Point every input-reading launch at another binding (device int64 batch-pointer word, fp32 maximum); the
        C-ABI copies the record into the kernel arguments at launch, so a graph captured afterwards keeps it.
        None: no binding -- the launches read the plan's own staging buffer and scale from their arguments, with no
        dependent pointer / maximum load ahead of the input window (the session's own launches, the bench path)."""
        for h in self.bind_holders:
            h.x, h.amax = (None, None) if ptr is None else (ptr.data_ptr(), amax.data_ptr())


def _propagate_shapes(layers, batch, h, w, ch):
    """Output NHWC shape of every layer (cheap symbolic pass over module types)."""
    shapes = []
    cur = (batch, h, w, ch)
    for m in layers:
        if m.f != -1:
            src = shapes[m.f] if isinstance(m.f, int) else [cur if j == -1 else shapes[j] for j in m.f]
        else:
            src = cur
        t = m.type
        mm = m[0] if isinstance(m, nn.Sequential) else m
        if t in ("Conv", "DWConv"):
            k, s, p, d = mm.conv.kernel_size[0], mm.conv.stride[0], mm.conv.padding[0], mm.conv.dilation[0]
            ho, wo = M.conv_out_hw(src[1], src[2], k, s, p, d)
            cur = (batch, ho, wo, (m[-1] if isinstance(m, nn.Sequential) else m).conv.out_channels)
        elif t == "DSConv":
            k, s, p, d = mm.dw.kernel_size[0], mm.dw.stride[0], mm.dw.padding[0], mm.dw.dilation[0]
            ho, wo = M.conv_out_hw(src[1], src[2], k, s, p, d)
            cur = (batch, ho, wo, (m[-1] if isinstance(m, nn.Sequential) else m).pw.out_channels)
        elif t in ("Bottleneck", "DSBottleneck"):
            cur = (batch, src[1], src[2], (m[-1] if isinstance(m, nn.Sequential) else m).cv2.conv.out_channels
                   if t == "Bottleneck" else (m[-1] if isinstance(m, nn.Sequential) else m).cv2.pw.out_channels)
        elif t in ("C2f", "DSC3k2", "A2C2f", "C3k2", "SPPF", "C2PSA", "PSA", "C2fCIB"):
            cur = (batch, src[1], src[2], mm.cv2.conv.out_channels)
        elif t == "SCDown":
            c = mm.cv2.conv
            cur = (batch, *M.conv_out_hw(src[1], src[2], c.kernel_size[0], c.stride[0], c.padding[0], c.dilation[0]),
                   c.out_channels)
        elif t == "CIB":
            cur = (batch, src[1], src[2], (m[-1] if isinstance(m, nn.Sequential) else m).cv1[4].conv.out_channels)
        elif t == "RepVGGDW":
            cur = src
        elif t in ("AAttn", "ABlock", "Attention", "PSABlock"):
            cur = src
        elif t == "nn.Upsample":
            cur = (batch, 2 * src[1], 2 * src[2], src[3])
        elif t in ("C3", "C3Ghost", "C3k"):
            cur = (batch, src[1], src[2], mm.cv3.conv.out_channels)
        elif t == "LSKblock":
            cur = src
        elif t == "HyperACE":
            cur = (batch, src[1][1], src[1][2], mm.cv2.conv.out_channels)
        elif t == "DySample":
            cur = (batch, 2 * src[1], 2 * src[2], src[3])
        elif t == "DownsampleConv":
            c = src[3] * 2 if not isinstance(mm.channel_adjust, nn.Identity) else src[3]
            cur = (batch, src[1] // 2, src[2] // 2, c)
        elif t == "FullPAD_Tunnel":
            cur = src[0]
        elif t == "Concat":
            cur = (batch, src[0][1], src[0][2], sum(s_[3] for s_ in src))
        elif t in _DETECT:
            cur = None
        elif not hasattr(mm, "emit"):  # a registered forward-only plugin: its output shape from a meta run
            cur = M.torch_out_shape(m, src)
        else:
            raise NotImplementedError(f"{t}: a registered module with emit() needs a shape rule here")
        shapes.append(cur)
    return shapes
