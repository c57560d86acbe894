"""Yardstick of the YOLOv10 baseline tests (test infrastructure; imports oracle/).

Plain-torch CPU restatements of SCDown (U/nn/modules/block.py:1088-1120), RepVGGDW (:756-815), CIB / C2fCIB (:818-880),
PSA (:970-1010) and v10Detect (U/nn/modules/head.py:768-817 on Detect's forward_end2end, :120-141), built on
oracle.model's Conv / C2f and yolo11_util's Attention / SPPF; Detect.postprocess (head.py:200-221) word for word; the
pinned-order selection the device kernel implements, as a plain sort; and builders of the baseline model through
oracle.model.DetectionModel with a dict cfg.  The classes are registered in oracle.model's tables in-process; no file
under oracle/ is edited.
"""

from __future__ import annotations

import copy
import json
import math
from pathlib import Path

import torch
import torch.nn as nn

import oracle.model as om
import yolo11_util as U11
from a2c2f_util import Upsample, fuse_, leg_bound, legs  # noqa: F401 (re-exported)
from oracle.model import C2f, Conv, Detect
from yolo11_util import SPPF, Attention

GOLDEN = Path(__file__).resolve().parent / "golden"


class SCDown(nn.Module):
    """block.py:1088-1120."""

    def __init__(self, c1, c2, k, s):
        super().__init__()
        self.cv1 = Conv(c1, c2, 1, 1)
        self.cv2 = Conv(c2, c2, k=k, s=s, g=c2, act=False)

    def forward(self, x):
        return self.cv2(self.cv1(x))


class RepVGGDW(nn.Module):
    """block.py:756-815."""

    def __init__(self, ed):
        super().__init__()
        self.conv = Conv(ed, ed, 7, 1, 3, g=ed, act=False)
        self.conv1 = Conv(ed, ed, 3, 1, 1, g=ed, act=False)
        self.dim = ed
        self.act = nn.SiLU()

    def forward(self, x):
        if not hasattr(self, "conv1"):  # forward_fuse
            return self.act(self.conv(x))
        return self.act(self.conv(x) + self.conv1(x))

    @torch.no_grad()
    def fuse(self):
        """:791-815."""
        conv = om.fuse_conv_and_bn(self.conv.conv, self.conv.bn)
        conv1 = om.fuse_conv_and_bn(self.conv1.conv, self.conv1.bn)
        conv_w, conv_b = conv.weight, conv.bias
        conv1_w, conv1_b = conv1.weight, conv1.bias
        conv1_w = torch.nn.functional.pad(conv1_w, [2, 2, 2, 2])
        final_conv_w = conv_w + conv1_w
        final_conv_b = conv_b + conv1_b
        conv.weight.data.copy_(final_conv_w)
        conv.bias.data.copy_(final_conv_b)
        self.conv = conv
        del self.conv1


class CIB(nn.Module):
    """block.py:818-850."""

    def __init__(self, c1, c2, shortcut=True, e=0.5, lk=False):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = nn.Sequential(
            Conv(c1, c1, 3, g=c1),
            Conv(c1, 2 * c_, 1),
            RepVGGDW(2 * c_) if lk else Conv(2 * c_, 2 * c_, 3, g=2 * c_),
            Conv(2 * c_, c2, 1),
            Conv(c2, c2, 3, g=c2),
        )
        self.add = shortcut and c1 == c2

    def forward(self, x):
        return x + self.cv1(x) if self.add else self.cv1(x)


class C2fCIB(C2f):
    """block.py:853-880."""

    def __init__(self, c1, c2, n=1, shortcut=False, lk=False, g=1, e=0.5):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(CIB(self.c, self.c, shortcut, e=1.0, lk=lk) for _ in range(n))


class PSA(nn.Module):
    """block.py:970-1010."""

    def __init__(self, c1, c2, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = Conv(2 * self.c, c1, 1)
        self.attn = Attention(self.c, attn_ratio=0.5, num_heads=self.c // 64)
        self.ffn = nn.Sequential(Conv(self.c, self.c * 2, 1), Conv(self.c * 2, self.c, 1, act=False))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), dim=1)
        b = b + self.attn(b)
        b = b + self.ffn(b)
        return self.cv2(torch.cat((a, b), 1))


def postprocess(preds: torch.Tensor, max_det: int, nc: int = 80) -> torch.Tensor:
    """Detect.postprocess, head.py:200-221, word for word."""
    batch_size, anchors, _ = preds.shape  # i.e. shape(16,8400,84)
    boxes, scores = preds.split([4, nc], dim=-1)
    index = scores.amax(dim=-1).topk(min(max_det, anchors))[1].unsqueeze(-1)
    boxes = boxes.gather(dim=1, index=index.repeat(1, 1, 4))
    scores = scores.gather(dim=1, index=index.repeat(1, 1, nc))
    scores, index = scores.flatten(1).topk(min(max_det, anchors))
    i = torch.arange(batch_size)[..., None]  # batch indices
    return torch.cat([boxes[i, index // nc], scores[..., None], (index % nc)[..., None].float()], dim=-1)


class v10Detect(Detect):  # noqa: N801 (reference name)
    """head.py:768-817 on Detect.forward_end2end (:120-141): eval mode only.  ``dense`` = True returns the decoded
    one2one map y [B, 4+nc, A] (xyxy rows) in place of its postprocess -- what the parity tests compare."""

    end2end = True
    max_det = 300
    dense = False

    def __init__(self, nc=80, ch=(), legacy=False):
        super().__init__(nc, ch, legacy)
        c3 = max(ch[0], min(self.nc, 100))
        self.cv3 = nn.ModuleList(
            nn.Sequential(
                nn.Sequential(Conv(x, x, 3, g=x), Conv(x, c3, 1)),
                nn.Sequential(Conv(c3, c3, 3, g=c3), Conv(c3, c3, 1)),
                nn.Conv2d(c3, self.nc, 1),
            )
            for x in ch
        )
        self.one2one_cv2 = copy.deepcopy(self.cv2)
        self.one2one_cv3 = copy.deepcopy(self.cv3)

    def bias_init(self):
        """head.py:183-194."""
        super().bias_init()
        for a, b, s in zip(self.one2one_cv2, self.one2one_cv3, self.stride):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[: self.nc] = math.log(5 / self.nc / (640 / s) ** 2)

    def _inference(self, x):
        """Detect._inference (head.py:143-181) with decode_bboxes' xywh=False of an end2end head (:196-198)."""
        B = x[0].shape[0]
        x_cat = torch.cat([xi.view(B, self.no, -1) for xi in x], 2)
        anchors, strides = (t.transpose(0, 1) for t in om.make_anchors([xi.shape[2:] for xi in x], self.stride, 0.5))
        box, cls = x_cat.split((self.reg_max * 4, self.nc), 1)
        dbox = om.dist2bbox(self.dfl(box), anchors.unsqueeze(0), xywh=False, dim=1) * strides
        return torch.cat((dbox, cls.sigmoid()), 1)

    def forward(self, x):
        x = list(x)
        one2one = [torch.cat((self.one2one_cv2[i](x[i]), self.one2one_cv3[i](x[i])), 1) for i in range(self.nl)]
        for i in range(self.nl):
            x[i] = torch.cat((self.cv2[i](x[i]), self.cv3[i](x[i])), 1)
        y = self._inference(one2one)
        if not self.dense:
            y = postprocess(y.permute(0, 2, 1), self.max_det, self.nc)
        return y, {"one2many": x, "one2one": one2one}


# ----------------------------------------------------------------------------- the pinned-order selection
def select_pinned(boxes, scores, k_head, conf=0.0, max_det=300, classes=None, clip=None):
    """The device rule for one image, as a plain sort: boxes [A, 4] xyxy, scores [A, nc].  All (anchor, class) pairs
    with score > conf, ordered by (score descending, anchor * nc + class ascending); the first min(k_head, max_det);
    then the `classes` filter; boxes clipped to clip = (h, w).  Returns rows [m, 6] fp32."""
    A, nc = scores.shape
    flat = scores.reshape(-1)
    idx = torch.arange(A * nc)
    m = flat > conf
    return select_candidates(boxes[idx[m] // nc], flat[m], (idx[m] % nc).int(), idx[m].int(), k_head, max_det,
                             classes, clip)


def select_candidates(cbox, cscore, ccls, cidx, k_head, max_det=300, classes=None, clip=None):
    """The same over candidate lists (any order): cbox [n, 4], cscore [n], ccls [n], cidx [n]."""
    bits = cscore.contiguous().view(torch.int32).long()  # positive floats order like their bit patterns
    order = sorted(range(len(cscore)), key=lambda i: (-int(bits[i]), int(cidx[i])))[: min(k_head, max_det)]
    order = torch.tensor(order, dtype=torch.long)
    rows = torch.cat([cbox[order].float(), cscore[order, None].float(), ccls[order, None].float()], 1)
    if classes is not None:
        rows = rows[(rows[:, 5:6] == torch.tensor(list(classes), dtype=torch.float32)).any(1)]
    if clip is not None:
        rows[:, [0, 2]] = rows[:, [0, 2]].clamp(0, clip[1])
        rows[:, [1, 3]] = rows[:, [1, 3]].clamp(0, clip[0])
    return rows


def reference_tail(pred_rows, conf, max_det, classes=None):
    """non_max_suppression's six-column branch (U/utils/ops.py:224-228) for one image of postprocess' output."""
    out = pred_rows[pred_rows[:, 4] > conf][:max_det]
    if classes is not None:
        out = out[(out[:, 5:6] == torch.tensor(list(classes), dtype=out.dtype)).any(1)]
    return out


# ----------------------------------------------------------------------------- model builders
def register():
    """The YOLOv10 classes (and SPPF, nn.Upsample) in the oracle's parser tables (in-process)."""
    U11.register()
    for cls in (SCDown, RepVGGDW, CIB, C2fCIB, PSA, SPPF):
        om._CLASSES[cls.__name__] = cls
    om._C1C2.update({"SCDown", "PSA", "C2fCIB", "SPPF"})
    om._REPEAT_INSERT.add("C2fCIB")
    om._CLASSES["nn.Upsample"] = Upsample


def baseline_cfg(scale: str = "n", nc: int | None = None) -> dict:
    d = json.loads((GOLDEN / "yolov10.json").read_text())
    d["scale"] = scale
    if nc:
        d["nc"] = nc
    return d


def build_oracle(scale: str = "n", nc: int = 3):
    """The restated yolov10 model (eval, unfused) under torch.manual_seed(0) with trained-like BN.  The oracle's parser
    knows no v10Detect: the table is parsed with a Detect in its place, which is then replaced by the restated head
    (before the weights are drawn)."""
    from ydbl.utils.synthetic import trained_like_

    register()
    cfg = baseline_cfg(scale, nc)
    assert cfg["head"][-1][2] == "v10Detect"
    cfg["head"][-1][2] = "Detect"
    torch.manual_seed(0)
    o = om.DetectionModel(cfg, stride_probe=False)
    head = o.model[-1]
    ch = [seq[0].conv.in_channels for seq in head.cv2]
    new = v10Detect(head.nc, ch)
    new.i, new.f, new.type, new.n_ = head.i, head.f, "v10Detect", head.n_
    new.stride = head.stride
    new.bias_init()
    for mod in new.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.eps, mod.momentum = 1e-3, 0.03
    o.model[-1] = new
    o.eval()
    return trained_like_(o, 0)


def fuse_model(o):
    """BaseModel.fuse (U/nn/tasks.py:207-235) for the restated model: RepVGGDW.fuse first (modules() yields it before
    its Convs), then the oracle's Conv folding."""
    for m in o.modules():
        if isinstance(m, RepVGGDW) and hasattr(m, "conv1"):
            m.fuse()
    return o.fuse()


def fuse_module(m: nn.Module) -> nn.Module:
    """The same for a stand-alone restated module."""
    for r in m.modules():
        if isinstance(r, RepVGGDW) and hasattr(r, "conv1"):
            r.fuse()
    return fuse_(m)


def build_pair(scale: str = "n", nc: int = 3):
    """(product YOLO, fused fp32 restatement with a dense head) with identical weights, copied by
    load_state_dict(strict=True)."""
    from ydbl import YOLO

    o = build_oracle(scale, nc)
    p = YOLO(str(GOLDEN / f"yolov10{scale}.json"), nc=nc)
    p.model.load_state_dict(o.state_dict(), strict=True)
    f = fuse_model(copy.deepcopy(o))
    f.model[-1].dense = True
    return p, f
