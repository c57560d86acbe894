"""Yardsticks of the mask-mAP tests (test infrastructure; imports oracle/).

The reference's expressions evaluated by torch on the CPU: mask_iou (U/utils/metrics.py:137-153), the ground-truth
side of SegmentationValidator._process_batch(masks=True) (U/models/yolo/segment/val.py:204-213: the index map's
indicator, F.interpolate(bilinear, align_corners=False), > 0.5) and the whole of it on top of
oracle.metrics.match_predictions; the bit-plane layout restated with np.packbits; a brute-force integer
point-in-closed-polygon test for the dataset's rasteriser.  Everything is compared exactly.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.metrics import IOUV, match_predictions


def pack_bits(u8) -> np.ndarray:
    """0 / 1 planes [..., H, W] -> uint64 words [..., H, ceil(W / 64)]: bit j of word q = pixel 64 q + j, tail 0."""
    a = np.asarray(u8).astype(bool)
    pad = (-a.shape[-1]) % 64
    if pad:
        a = np.concatenate([a, np.zeros((*a.shape[:-1], pad), dtype=bool)], -1)
    by = np.packbits(a, axis=-1, bitorder="little")
    return np.ascontiguousarray(by).view("<u8")


def words_np(t: torch.Tensor) -> np.ndarray:
    """An int64 word tensor as uint64 numpy."""
    return t.cpu().contiguous().numpy().view(np.uint64)


def mask_iou_ref(mask1: torch.Tensor, mask2: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """U/utils/metrics.py:137-153 on fp32 CPU tensors."""
    intersection = torch.matmul(mask1, mask2.T).clamp_(0)
    union = (mask1.sum(1)[:, None] + mask2.sum(1)[None]) - intersection
    return intersection / (union + eps)


def gt_planes_ref(src: torch.Tensor, nl: int, overlap: bool, hw, values: bool = False) -> torch.Tensor:
    """val.py:204-212 for one image: src the index map [gh, gw] (overlap) or its planes [nl, gh, gw] -> fp32 0 / 1
    [nl, H, W]; values=True: the interpolated values before the > 0.5."""
    if overlap:
        index = torch.arange(nl).view(nl, 1, 1) + 1
        g = torch.where(src[None].repeat(nl, 1, 1) == index, 1.0, 0.0)
    else:
        g = (src != 0).float()
    if nl == 0:
        return torch.zeros((0, *hw))
    if tuple(g.shape[1:]) != tuple(hw):
        g = F.interpolate(g[None], tuple(hw), mode="bilinear", align_corners=False)[0]
        if values:
            return g
        g = g.gt_(0.5)
    return g


def tp_m_ref(det, counts, pred_masks, offs, gt_masks, gt_cls, bidx, overlap=True, single_cls=False, iouv=IOUV):
    """update_metrics' tp_m blocks (val.py:99-142) for a batch on the CPU: det [B, max_det, 6], counts list,
    pred_masks [sum(counts), H, W] 0 / 1 with offs [B + 1] (session.masks), gt_masks the index map [B, gh, gw]
    (overlap) or planes [N, gh, gw] in label order, gt_cls [N], bidx [N].  Returns the list of bool blocks in the
    validator's order, and the list of the per-image IoU matrices."""
    blocks, ious = [], []
    bidx = torch.as_tensor(bidx).reshape(-1).long()
    for si in range(det.shape[0]):
        npr = int(counts[si])
        sel = bidx == si
        cls = torch.as_tensor(gt_cls).reshape(-1).float()[sel]
        nl = len(cls)
        if npr == 0:
            if nl:
                blocks.append(torch.zeros(0, len(iouv), dtype=torch.bool))
            continue
        pm = pred_masks[offs[si]:offs[si + 1]].float()
        pc = det[si, :npr, 5].clone()
        if single_cls:
            pc[:] = 0
        if nl == 0:
            blocks.append(torch.zeros(npr, len(iouv), dtype=torch.bool))
            continue
        src = gt_masks[si] if overlap else gt_masks[sel]
        g = gt_planes_ref(torch.as_tensor(src), nl, overlap, pm.shape[1:])
        iou = mask_iou_ref(g.reshape(nl, -1), pm.reshape(npr, -1))
        ious.append(iou)
        blocks.append(match_predictions(pc, cls, iou, iouv))
    return blocks, ious


def has_tie(iou: torch.Tensor, gt_cls, pred_cls, above: float = 0.5) -> bool:
    """Whether a detection has two same-class labels with bit-equal IoU >= above (the match rule's one freedom)."""
    m = (iou * (torch.as_tensor(gt_cls)[:, None] == torch.as_tensor(pred_cls)[None])).numpy()
    for d in range(m.shape[1]):
        v = m[:, d][m[:, d] >= above]
        if len(v) != len(np.unique(v)):
            return True
    return False


def blob_planes(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """n uint8 0 / 1 planes [n, h, w], each a filled ellipse; neighbours overlap."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((n, h, w), dtype=np.uint8)
    for i in range(n):
        cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
        ry, rx = rng.uniform(0.1, 0.4) * h, rng.uniform(0.1, 0.4) * w
        out[i] = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    return out


def index_map(planes: np.ndarray) -> np.ndarray:
    """uint8 planes [n, h, w] -> the overlap index map [h, w]: plane l as value l + 1, a later one overwriting."""
    out = np.zeros(planes.shape[1:], dtype=np.uint8)
    for l, p in enumerate(planes):
        out[p != 0] = l + 1
    return out


def point_in_closed_polygon(x: int, y: int, pts) -> bool:
    """Brute force, integers only: on an edge, or inside by the even-odd rule (a ray to +x, edges half-open in y)."""
    n = len(pts)
    inside = False
    for i in range(n):
        (ax, ay), (bx, by) = pts[i], pts[(i + 1) % n]
        if (bx - ax) * (y - ay) == (by - ay) * (x - ax) and min(ax, bx) <= x <= max(ax, bx) \
                and min(ay, by) <= y <= max(ay, by):
            return True
        if (ay <= y) != (by <= y):
            # x-coordinate of the crossing is ax + (y - ay) (bx - ax) / (by - ay); is it right of x?
            num, den = (y - ay) * (bx - ax), by - ay
            if den < 0:
                num, den = -num, -den
            if (x - ax) * den < num:
                inside = not inside
    return inside


def polygon_mask_ref(hw, poly) -> np.ndarray:
    pts = [(int(px), int(py)) for px, py in np.asarray(poly, dtype=np.float32).reshape(-1, 2).astype(np.int32)]
    out = np.zeros(hw, dtype=np.uint8)
    if pts:
        for y in range(hw[0]):
            for x in range(hw[1]):
                out[y, x] = point_in_closed_polygon(x, y, pts)
    return out


def downsample_ref(mask: np.ndarray) -> np.ndarray:
    h, w = mask.shape[0] // 4, mask.shape[1] // 4
    out = np.zeros((h, w), dtype=np.uint8)
    for Y in range(h):
        for X in range(w):
            out[Y, X] = int(mask[4 * Y + 1:4 * Y + 3, 4 * X + 1:4 * X + 3].sum()) >= 2
    return out
