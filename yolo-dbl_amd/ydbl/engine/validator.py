"""Detection validation (mAP) for the mAP@0.5 acceptance check.

Follows BaseValidator.__call__ (U/engine/validator.py:107-220) and DetectionValidator
(U/models/yolo/detect/val.py:50-227): NMS with multi_label=True at conf 0.001, iou 0.7 (val.py:92-102) —
run on the GPU in the same hipGraph as the forward —, TP matrix at IoU 0.5:0.95 (val.py:209-227 +
match_predictions) on the device with ydbl_match_predictions right behind NMS, then ap_per_class on the host.

``data`` is either
- a data YAML / its folder / its parsed dict (check_det_dataset), or an image directory / *.txt list: a
  YOLO-format dataset read by ydbl.engine.dataset (rect batches, letterboxed on the GPU by ydbl_letterbox) and
  matched in native image space after scale_boxes(ratio_pad) (val.py:104-123), like the reference; or
- an iterable of in-memory batches ``{"img": float [B,3,H,W] (0..1 or 0..255), "cls": [N], "bboxes": [N,4]
  xyxy pixels of the input image, "batch_idx": [N]}`` (boxes clipped to the input, gain 1 / pad 0).

Beside the mean scalars the validator reports what the reference's does: ``metrics.confusion_matrix`` (counted on
the device by ydbl_confusion_matrix on the tensors the TP matrix is matched on; ``plots=False`` skips it, as in
the reference — no image files are written either way), the per-class table (``nt_per_class``, ``nt_per_image``,
``seen``, ``print_results()``), and for dataset-backed runs with ``save_dir`` the ``predictions.json`` rows of
``save_json`` and the ``labels/<stem>.txt`` files of ``save_txt`` / ``save_conf``.

``coco_eval=True`` adds the COCO protocol the reference reaches through pycocotools (val.py:297-337): the per-image
matching of COCOeval.evaluateImg runs on the device (ydbl_coco_match, one launch per batch behind the two above, on
the same tensors and label grouping), COCOeval.accumulate / summarize on the host (utils/metrics.py):
``metrics.coco_stats`` (the 12 stats), ``metrics.coco_eval`` (precision / recall / scores in COCOeval's layout),
``coco_summary()`` and, with ``save_dir``, ``coco_stats.csv``.  pycocotools itself is not used.  One difference
from the reference path: that one evaluates the predictions.json rows (bbox rounded to 3 decimals, score to 5), this
the unrounded fp32 boxes and scores.  The Ultralytics fields above are not touched by it.

``loss=True`` adds the validation loss the reference's trainer logs (U/engine/validator.py:185, :205): the session
keeps dense Detect levels and runs ydbl_detect_loss behind each batch's forward, in the same graph, on the labels in
letterboxed space (dataset batches: the normalised xywh they already carry; tensor batches: their xyxy pixels).  Each
batch's numbers stay on the device until the end (one read-back); ``metrics.val_loss`` is their sum over the number of
batches,
``metrics.results_dict`` gains ``val/box_loss`` / ``val/cls_loss`` / ``val/dfl_loss``, ``image_loss`` is the
[images, 3] per-image table in dataset order (each batch's rows add up to that batch's values) and, with
``save_dir``, ``val_loss.csv`` holds both.  Without the flag none of this exists: nothing is compiled, launched,
copied or synchronised for it.

A segmentation model whose batches carry ground-truth ``"masks"`` (or whose dataset has polygon labels) is scored by
SegmentationValidator below: the same run plus the mask TP matrix ``stats["tp_m"]``, matched on the device on bit
planes, and SegmentMetrics.

A pose model whose batches carry ground-truth ``"keypoints"`` (or whose dataset has pose label rows) is scored by
PoseValidator: the same run plus the keypoint TP matrix ``stats["tp_p"]`` -- OKS on the device (ydbl_kpt_oks), then
ydbl_match_iou -- and PoseMetrics.
"""

from __future__ import annotations

import ctypes as C
import json
import math
import os
from pathlib import Path

import numpy as np
import torch

from .. import _lib
from ..utils.metrics import (COCO_AREA_RNG, COCO_IOU_THRS, COCO_MAX_DETS, IOUV, LOGGER, OKS_SIGMA, ConfusionMatrix,
                             DetMetrics, PoseMetrics, SegmentMetrics, coco_summary_lines)
from .model import load_tensor_source, select_device


def group_labels(gt_box, gt_cls, batch_idx, b: int, dev):
    """A batch's labels grouped by image for the device kernels: (gt_box fp32 [N, 4], gt_cls fp32 [N], gt_ofs
    int32 [b + 1], N) on dev.  Labels may arrive in any image order; the grouping is stable, so each image keeps
    its own order, like the reference's per-image slice ``batch_idx == si``."""
    bidx = torch.as_tensor(batch_idx).reshape(-1).long().cpu()
    order = torch.argsort(bidx, stable=True)
    ofs = torch.zeros(b + 1, dtype=torch.int32)
    if len(bidx):
        if int(bidx.min()) < 0 or int(bidx.max()) >= b:
            raise ValueError(f"batch_idx must be in [0, {b})")
        ofs[1:] = torch.cumsum(torch.bincount(bidx, minlength=b), 0).to(torch.int32)
    boxes = torch.as_tensor(gt_box).reshape(-1, 4).float().cpu()[order].to(dev).contiguous()
    cls = torch.as_tensor(gt_cls).reshape(-1).float().cpu()[order].to(dev).contiguous()
    return boxes, cls, ofs.to(dev), len(bidx)


def confusion_batch(det: torch.Tensor, count: torch.Tensor, gt_box, gt_cls, batch_idx, cm,
                    single_cls: bool = False, grouped=None) -> None:
    """Add one batch to a ydbl.utils.metrics.ConfusionMatrix on the device (ydbl_confusion_matrix): one launch
    for ConfusionMatrix.process_batch (U/utils/metrics.py:326-382) over every image, as update_metrics calls it
    (U/models/yolo/detect/val.py:140-159).  det / count / labels as for match_batch (``grouped``: the result of
    group_labels, to share one grouping with it); single_cls counts every detection as class 0 (val.py:149-150).
    Nothing is read back: ``cm.matrix`` does that."""
    if det.device.type != "cuda":
        raise RuntimeError("confusion_batch runs on the GPU (ydbl_confusion_matrix); got a CPU tensor")
    dev = det.device
    b, max_det = det.shape[0], det.shape[1]
    boxes, cls, ofs, n_gt = grouped or group_labels(gt_box, gt_cls, batch_idx, b, dev)
    det = det.float().contiguous()
    if single_cls:
        det = det.clone()
        det[..., 5] = 0
    count = count.to(dev, torch.int32).contiguous()
    acc, invalid = cm.buffers(dev)
    ws = torch.empty(int(_lib.lib.ydbl_confusion_workspace(b, max_det, n_gt)), dtype=torch.uint8, device=dev)
    d = _lib.ConfusionDesc(det.data_ptr(), count.data_ptr(), b, max_det, boxes.data_ptr() if n_gt else None,
                           cls.data_ptr() if n_gt else None, ofs.data_ptr(), n_gt, cm.nc, cm.conf, cm.iou_thres,
                           acc.data_ptr(), invalid.data_ptr(), ws.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib.ydbl_confusion_matrix(C.byref(d), stream), "ydbl_confusion_matrix")


def match_batch(det: torch.Tensor, count: torch.Tensor, gt_box: torch.Tensor, gt_cls: torch.Tensor,
                batch_idx: torch.Tensor, iouv: torch.Tensor = IOUV, single_cls: bool = False,
                grouped=None) -> torch.Tensor:
    """TP matrix of one batch on the device (ydbl_match_predictions).

    det fp32 [B, max_det, 6] and count int32 [B] as NMS leaves them; labels gt_box [N, 4] xyxy,
    gt_cls [N], batch_idx [N] in any image order (kept in order within an image, like the
    reference's per-image label slice).  Returns bool [B, max_det, len(iouv)] on det's device;
    rows >= count are False.  Same results as DetectionValidator._process_batch
    (U/models/yolo/detect/val.py:209-227) per image.
    """
    if det.device.type != "cuda":
        raise RuntimeError("match_batch runs on the GPU (ydbl_match_predictions); got a CPU tensor")
    dev = det.device
    b, max_det = det.shape[0], det.shape[1]
    boxes, cls, ofs, n_gt = grouped or group_labels(gt_box, gt_cls, batch_idx, b, dev)
    iouv_d = iouv.float().to(dev).contiguous()
    det = det.float().contiguous()
    count = count.to(dev, torch.int32).contiguous()
    out = torch.empty((b, max_det, len(iouv)), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(_lib.lib.ydbl_match_workspace(b, max_det, n_gt, len(iouv))), dtype=torch.uint8, device=dev)
    d = _lib.MatchDesc(det.data_ptr(), count.data_ptr(), b, max_det, boxes.data_ptr() if n_gt else None,
                       cls.data_ptr() if n_gt else None, ofs.data_ptr(), n_gt, iouv_d.data_ptr(), len(iouv),
                       int(bool(single_cls)), out.data_ptr(), ws.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib.ydbl_match_predictions(C.byref(d), stream), "ydbl_match_predictions")
    return out.bool()


def match_iou_batch(det: torch.Tensor, count: torch.Tensor, iou: torch.Tensor, gt_cls: torch.Tensor,
                    gt_ofs: torch.Tensor, iouv: torch.Tensor = IOUV, single_cls: bool = False) -> torch.Tensor:
    """match_batch on a given IoU matrix (ydbl_match_iou): iou fp32 [n_gt, max_det] on the device, row g = label g
    (grouped order, gt_cls / gt_ofs as group_labels returns them) against the slots of its own image -- what
    ydbl_mask_iou writes.  det supplies the class column.  Returns bool [B, max_det, len(iouv)]; same results as
    SegmentationValidator._process_batch(masks=True) (U/models/yolo/segment/val.py:173-217) per image."""
    if det.device.type != "cuda":
        raise RuntimeError("match_iou_batch runs on the GPU (ydbl_match_iou); got a CPU tensor")
    dev = det.device
    b, max_det = det.shape[0], det.shape[1]
    n_gt = int(gt_cls.numel())
    if tuple(iou.shape) != (n_gt, max_det):
        raise ValueError(f"iou must be [{n_gt}, {max_det}], got {tuple(iou.shape)}")
    iouv_d = iouv.float().to(dev).contiguous()
    det = det.float().contiguous()
    iou = iou.float().contiguous()
    count = count.to(dev, torch.int32).contiguous()
    out = torch.empty((b, max_det, len(iouv)), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(_lib.lib.ydbl_match_workspace(b, max_det, n_gt, len(iouv))), dtype=torch.uint8, device=dev)
    d = _lib.MatchIouDesc(det.data_ptr(), count.data_ptr(), b, max_det, iou.data_ptr() if n_gt else None,
                          gt_cls.data_ptr() if n_gt else None, gt_ofs.data_ptr(), n_gt, iouv_d.data_ptr(), len(iouv),
                          int(bool(single_cls)), out.data_ptr(), ws.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib.ydbl_match_iou(C.byref(d), stream), "ydbl_match_iou")
    return out.bool()


def coco_batch(det: torch.Tensor, count: torch.Tensor, gt_box, gt_cls, batch_idx, nc: int, single_cls: bool = False,
               grouped=None, iou_thrs=COCO_IOU_THRS, area_rng=COCO_AREA_RNG, max_dets: int = COCO_MAX_DETS[-1]) -> dict:
    """COCO-protocol matching of one batch on the device (ydbl_coco_match): one launch for COCOeval.evaluateImg over
    every (image, category, area range, IoU threshold).  det / count / labels as for match_batch (``grouped``: the
    result of group_labels, to share one grouping with it).  Returns device tensors: ``rank`` int32 [B, max_det]
    (the row's place in its image's category list by score, -1 when it takes no part), ``matched`` / ``ignored``
    int32 [B, max_det, A] (bit t: at iou_thrs[t]), ``gt_ignore`` uint8 [N, A] (labels in grouped order) and
    ``invalid`` int32 [B] (rows whose class is outside [0, nc)).  Nothing is read back."""
    if det.device.type != "cuda":
        raise RuntimeError("coco_batch runs on the GPU (ydbl_coco_match); got a CPU tensor")
    dev = det.device
    b, max_det = det.shape[0], det.shape[1]
    boxes, cls, ofs, n_gt = grouped or group_labels(gt_box, gt_cls, batch_idx, b, dev)
    det = det.float().contiguous()
    count = count.to(dev, torch.int32).contiguous()
    thr = np.ascontiguousarray(iou_thrs, dtype=np.float64)
    rng = np.ascontiguousarray(area_rng, dtype=np.float64).reshape(-1, 2)
    A = len(rng)
    out = {"rank": torch.empty((b, max_det), dtype=torch.int32, device=dev),
           "matched": torch.empty((b, max_det, A), dtype=torch.int32, device=dev),
           "ignored": torch.empty((b, max_det, A), dtype=torch.int32, device=dev),
           "gt_ignore": torch.empty((n_gt, A), dtype=torch.uint8, device=dev),
           "invalid": torch.empty(b, dtype=torch.int32, device=dev)}
    nws = int(_lib.lib.ydbl_coco_workspace(b, max_det, n_gt, nc))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws > 0 else None
    d = _lib.CocoDesc(det.data_ptr(), count.data_ptr(), b, max_det, boxes.data_ptr() if n_gt else None,
                      cls.data_ptr() if n_gt else None, ofs.data_ptr(), n_gt, int(bool(single_cls)), int(nc),
                      thr.ctypes.data, len(thr), rng.ctypes.data, A, int(max_dets), out["rank"].data_ptr(),
                      out["matched"].data_ptr(), out["ignored"].data_ptr(),
                      out["gt_ignore"].data_ptr() if n_gt else None, out["invalid"].data_ptr(),
                      ws.data_ptr() if ws is not None else None)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.lib.ydbl_coco_match(C.byref(d), stream), "ydbl_coco_match")
    return out


def coco_host_record(det, out, gt_cls, nc: int, single_cls: bool) -> dict:
    """One batch's coco_batch outputs as the numpy record coco_accumulate reads: det [B, max_det, 6] and ``out`` on
    the host, gt_cls the labels' classes in grouped order."""
    det = det.float().numpy()
    c = det[..., 5]
    gc = np.asarray(gt_cls, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        cls = np.where((c > -1) & (c < nc), c, -1).astype(np.int64)  # the kernel's rule: truncation inside (-1, nc)
        gcls = np.where((gc > -1) & (gc < nc), gc, -1).astype(np.int64)
    if single_cls:
        cls, gcls = np.zeros_like(cls), np.zeros_like(gcls)
    return {"score": det[..., 4], "cls": cls, "rank": out["rank"].numpy(), "matched": out["matched"].numpy(),
            "ignored": out["ignored"].numpy(), "gt_cls": gcls, "gt_ignore": out["gt_ignore"].numpy().astype(bool)}


def val_source(data, split: str, n_names: int):
    """What a dataset-backed val() reads: (image source of the split, class count) from a data YAML / its folder /
    its parsed dict, or the image directory / *.txt list itself."""
    from .dataset import check_det_dataset

    is_yaml = isinstance(data, dict) or str(data).rsplit(".", 1)[-1] in {"yaml", "yml"} or (
        Path(data).is_dir() and (list(Path(data).glob("*.yaml")) or not _has_images(Path(data))))
    if not is_yaml:
        return data, n_names
    info = check_det_dataset(data)
    src = info.get(split)
    if not src:
        raise FileNotFoundError(f"dataset has no '{split}' split")
    return src, info["nc"]


class DetectionValidator:
    stat_keys = ("tp", "conf", "pred_cls", "target_cls")
    with_masks = False
    tp2_key = "tp_m"  # the second TP matrix of a subclass (_match_masks): "tp_m" for masks, "tp_p" for keypoints

    def __init__(self, model, args):
        self.model = model
        self.args = args
        self.iouv = IOUV
        self.metrics = DetMetrics(names=model.names)

    def __call__(self, data):
        if data is None:
            raise ValueError("val(data=...) needs a data YAML, an image folder, or an iterable of batches")
        dev = select_device(self.args.get("device"))
        self.stats = {k: [] for k in self.stat_keys}
        self.target_img = []  # per image with labels or predictions: its distinct label classes (val.py:139)
        self.seen = 0
        self.nc = len(self.model.names)
        self.confusion_matrix = ConfusionMatrix(nc=self.nc, conf=self.args["conf"])  # val.py:83
        self.jdict = []
        self.coco_batches = []  # coco_eval=True: one host record per batch (coco_host_record)
        self.coco_invalid = 0
        self.save_dir = Path(self.args["save_dir"]) if self.args.get("save_dir") else None
        if self.args.get("loss"):
            self.loss_batches = []  # per batch: device fp32 [3 + 1 + 3 * b] (loss | target_scores_sum | per_image)
        if isinstance(data, (str, os.PathLike, dict)):
            self._run_dataset(data, dev)
        else:
            for batch in data:
                self._run_tensor_batch(batch, dev)
        st = {k: torch.cat(v, 0).numpy() if v else np.zeros((0, 10) if k in ("tp", "tp_m", "tp_p") else 0)
              for k, v in self.stats.items()}
        # get_stats (val.py:179-187)
        self.nt_per_class = np.bincount(st["target_cls"].astype(int), minlength=self.nc)
        timg = torch.cat(self.target_img).numpy() if self.target_img else np.zeros(0)
        self.nt_per_image = np.bincount(timg.astype(int), minlength=self.nc)
        if len(st["tp"]) and st["tp"].any():
            self.metrics.process(*(st[k] for k in self.stat_keys))
        self.metrics.confusion_matrix = self.confusion_matrix  # finalize_metrics (val.py:174-177)
        if self.args.get("coco_eval"):
            self._finish_coco()
        if self.args.get("loss"):
            self._finish_loss()
        if self.save_dir is not None and self.args.get("save_json") and self.jdict:
            self.save_dir.mkdir(parents=True, exist_ok=True)
            with open(self.save_dir / "predictions.json", "w") as f:  # U/engine/validator.py:205-208
                json.dump(self.jdict, f)
        if self.args.get("verbose"):
            print("\n".join([self.get_desc(), *self.print_results()]))
            if self.args.get("coco_eval"):
                print("\n".join(self.coco_summary()))
        return self.metrics

    def _finish_coco(self):
        """COCOeval.accumulate + summarize over the batches' device matching, and coco_stats.csv under save_dir."""
        if self.coco_invalid:
            LOGGER.warning(f"coco_eval: {self.coco_invalid} detections had a class outside [0, {self.nc}) and were "
                           "left out")
        self.metrics.process_coco(self.coco_batches, self.nc)
        if self.save_dir is not None:
            self.save_dir.mkdir(parents=True, exist_ok=True)
            with open(self.save_dir / "coco_stats.csv", "w") as f:
                f.write(",".join(self.metrics.coco_stat_names) + "\n")
                f.write(",".join(repr(float(v)) for v in self.metrics.coco_stats) + "\n")

    def _finish_loss(self):
        """The mean over the batches (U/engine/validator.py:205: loss / len(dataloader)), the per-image table and
        val_loss.csv under save_dir.  The one read-back of the loss path."""
        rows = [t.cpu() for t in self.loss_batches]
        self.batch_loss = torch.stack([r[:3] for r in rows]) if rows else torch.zeros((0, 3))
        self.image_loss = torch.cat([r[4:].view(-1, 3) for r in rows]) if rows else torch.zeros((0, 3))
        total = torch.zeros(3)
        for r in rows:  # the reference's running sum, in batch order
            total += r[:3]
        self.metrics.val_loss = (total / max(len(rows), 1)).tolist()
        if self.save_dir is not None:
            self.save_dir.mkdir(parents=True, exist_ok=True)
            files = getattr(self, "loss_files", None) or [f"image{i}" for i in range(len(self.image_loss))]
            with open(self.save_dir / "val_loss.csv", "w") as f:
                f.write("image,box_loss,cls_loss,dfl_loss\n")
                f.write("all," + ",".join(repr(float(v)) for v in self.metrics.val_loss) + "\n")
                for name, row in zip(files, self.image_loss.tolist()):
                    f.write(f"{name}," + ",".join(repr(float(v)) for v in row) + "\n")

    def _launch(self, s, im, gt):
        """One batch through the session; with loss=True the padded labels go into the loss step's buffer first and
        the step's outputs are copied aside on the device (no sync)."""
        if gt is not None:
            s.load_labels(gt)
        out = s(im)
        if gt is not None:
            self.loss_batches.append(s.loss.out.clone())
        return out

    def _loss_labels(self, bidx, cls, boxes, b, scale, xywh):
        if not self.args.get("loss"):
            return None
        from ..utils.loss import MAX_LABELS, pad_targets

        nc = self.model.model.nc
        if self.args.get("single_cls"):  # one class (val.py:149-150): the labels the validator scores
            cls = torch.zeros_like(torch.as_tensor(cls).reshape(-1).float())
        return pad_targets(bidx, cls, boxes, b, scale, self.args.get("max_labels", MAX_LABELS), xywh=xywh, nc=nc)

    def coco_summary(self):
        """The twelve lines COCOeval.summarize prints, from the last val(coco_eval=True)."""
        if self.metrics.coco_eval is None:
            raise RuntimeError("coco_summary() needs a val(coco_eval=True) run")
        return coco_summary_lines(self.metrics.coco_eval)

    def get_desc(self):
        """val.py:88-90: the table header of this fork (mAP75 is its fifth metric column)."""
        return ("%22s" + "%11s" * 7) % ("Class", "Images", "Instances", "Box(P", "R", "mAP50", "mAP75", "mAP50-95)")

    def print_results(self):
        """val.py:189-201: the 'all' line and, for nc > 1, one line per class that has labels; logged to the
        'ydbl' logger and returned (val(verbose=True) prints them under get_desc())."""
        pf = "%22s" + "%11i" * 2 + "%11.3g" * len(self.metrics.keys)
        lines = [pf % ("all", self.seen, self.nt_per_class.sum(), *self.metrics.mean_results())]
        if self.nt_per_class.sum() == 0:
            LOGGER.warning("no labels found in the val set, can not compute metrics without labels")
        if self.nc > 1:
            for i, c in enumerate(self.metrics.ap_class_index):
                lines.append(pf % (self.model.names[c], self.nt_per_image[c], self.nt_per_class[c],
                                   *self.metrics.class_result(i)))
        for ln in lines:
            LOGGER.info(ln)
        return lines

    def _session(self, b, h, w, dev, clip):
        a = self.args
        return self.model.session(b, h, w, half=a.get("half", False), conf=a["conf"], iou=a["iou"],
                                  max_det=a.get("max_det", 300), multi_label=True,
                                  agnostic=a.get("agnostic_nms", False) or a.get("single_cls", False), device=dev,
                                  fp8=a.get("fp8", False), clip=clip, streams=a.get("streams") or 1,
                                  fp8_calibration=a.get("fp8_calibration"), augment=a.get("augment", False),
                                  **({"loss": {"max_labels": a["max_labels"]} if a.get("max_labels") else True}
                                     if a.get("loss") else {}))

    def _match_masks(self, det_d, cnt_d, grouped, bidx, single):
        """The second TP matrix of the batch (masks, keypoints) on the device, launched behind the box matching; None
        here: a subclass's step."""
        return None

    def _dataset_kw(self) -> dict:
        """What the subclass asks of YOLOValDataset beside the boxes."""
        return {"masks": True} if self.with_masks else {}

    def _native_extra(self, hb, gain, pad, ori):
        """A dataset batch's further predictions and labels brought to native space (device gain [B], pad [B, 2],
        ori (w, h) [B, 2]); nothing here."""

    def _json_rows(self, pred, si, im_file) -> list:
        return pred_to_json(pred, im_file)

    def _save_txt(self, pred, si, shape, file):
        save_one_txt(pred, bool(self.args.get("save_conf", False)), shape, self.model.names, file)

    def _run_tensor_batch(self, batch, dev):
        if not self.with_masks and "masks" in batch and getattr(self.model.model, "segment", False):
            raise ValueError("val(): only some batches carry 'masks' (the first one does not); mask metrics need "
                             "them in every batch")
        im = load_tensor_source(batch["img"], int(self.model.model.stride.max())).to(dev).float()
        b, _, h, w = im.shape
        gt = self._loss_labels(batch["batch_idx"], batch["cls"], batch["bboxes"], b, None, xywh=False)
        det_d, cnt_d = self._launch(self._session(b, h, w, dev, clip=True), im, gt)
        self._update(det_d, cnt_d, torch.as_tensor(batch["bboxes"]).cpu().float().reshape(-1, 4),
                     torch.as_tensor(batch["cls"]).cpu().float().reshape(-1),
                     torch.as_tensor(batch["batch_idx"]).cpu().reshape(-1))

    def _run_dataset(self, data, dev):
        """A YOLO-format dataset: rect batches letterboxed on the GPU, predictions and labels in native space."""
        from .dataset import YOLOValDataset
        from .preprocess import letterbox_frames

        a = self.args
        stride = int(self.model.model.stride.max())
        src, num_cls = val_source(data, a.get("split", "val"), len(self.model.names))
        imgsz = a.get("imgsz", 640)
        imgsz = imgsz if isinstance(imgsz, int) else max(imgsz)
        imgsz = max(math.ceil(imgsz / stride) * stride, stride)  # check_imgsz (U/utils/checks.py)
        ds = YOLOValDataset(src, imgsz=imgsz, batch_size=a.get("batch", 16), stride=stride, rect=a.get("rect", True),
                            single_cls=a.get("single_cls", False), classes=a.get("classes"), num_cls=num_cls,
                            workers=a.get("workers", 8), **self._dataset_kw())
        self.dataset = ds
        for hb in ds.batches():
            H, W = hb["shape"]
            b = len(hb["frames"])
            im = letterbox_frames(hb["frames"], hb["meta"], H, W, device=dev)
            # the reference's val NMS does not clip: scale_boxes clips to the original image afterwards
            gt = self._loss_labels(hb["batch_idx"], hb["cls"], hb["bboxes"], b, (W, H, W, H), xywh=True)
            if self.with_masks:
                self._gt_masks = hb["masks"]
            if gt is not None:
                self.__dict__.setdefault("loss_files", []).extend(str(f) for f in hb["im_file"])
            det_d, cnt_d = self._launch(self._session(b, H, W, dev, clip=False), im, gt)
            det_n = det_d.clone()
            gain = torch.tensor([rp[0][0] for rp in hb["ratio_pad"]], dtype=torch.float32, device=dev)
            pad = torch.tensor([rp[1] for rp in hb["ratio_pad"]], dtype=torch.float32, device=dev)
            ori = torch.tensor([[s[1], s[0]] for s in hb["ori_shape"]], dtype=torch.float32, device=dev)
            _scale_clip(det_n[..., :4], pad[:, None, :], gain[:, None, None], ori[:, None, :])
            bidx = torch.from_numpy(hb["batch_idx"]).long()
            native = native_labels(hb)
            self._native_extra(hb, gain, pad, ori)
            self._update(det_n, cnt_d, native, torch.from_numpy(hb["cls"]).float(), bidx,
                         im_files=hb["im_file"], ori_shapes=hb["ori_shape"])

    def _update(self, det_d, cnt_d, box_all, cls_all, bidx, im_files=None, ori_shapes=None):
        """update_metrics (val.py:125-172) for one batch: device TP matrix and confusion counts (one launch each on
        one label grouping), host stats in image order, and for dataset batches the predictions.json rows / label
        files of save_json / save_txt."""
        b = det_d.shape[0]
        single = bool(self.args.get("single_cls", False))
        grouped = group_labels(box_all, cls_all, bidx, b, det_d.device)
        tp_all = match_batch(det_d, cnt_d, box_all, cls_all, bidx, self.iouv, single, grouped=grouped)
        tp_m_all = self._match_masks(det_d, cnt_d, grouped, bidx, single)
        if self.args.get("plots", True):  # val.py:144-145, :158-159
            confusion_batch(det_d, cnt_d, box_all, cls_all, bidx, self.confusion_matrix, single, grouped=grouped)
        coco = None
        if self.args.get("coco_eval"):
            coco = coco_batch(det_d, cnt_d, box_all, cls_all, bidx, self.nc, single, grouped=grouped)
        tp_all = tp_all.cpu()
        if tp_m_all is not None:
            tp_m_all = tp_m_all.cpu()  # with the box matrix: the batch's one read-back
        det, cnt = det_d.cpu(), cnt_d.cpu().tolist()
        if coco is not None:
            coco = {k: v.cpu() for k, v in coco.items()}
            self.coco_invalid += int(coco["invalid"].sum())
            by_image = torch.argsort(torch.as_tensor(bidx).reshape(-1).long(), stable=True)  # group_labels' order
            self.coco_batches.append(coco_host_record(det, coco, cls_all[by_image], self.nc, single))
        save = self.save_dir is not None and im_files is not None
        for si in range(b):
            self.seen += 1
            pred = det[si, : cnt[si]]
            cls = cls_all[bidx == si]
            nl, npr = len(cls), len(pred)
            if npr == 0:
                if nl:
                    self.stats["tp"].append(torch.zeros(0, len(self.iouv), dtype=torch.bool))
                    if tp_m_all is not None:  # segment/val.py:115-118: the (0, n_iou) block
                        self.stats[self.tp2_key].append(torch.zeros(0, len(self.iouv), dtype=torch.bool))
                    self.stats["conf"].append(torch.zeros(0))
                    self.stats["pred_cls"].append(torch.zeros(0))
                    self.stats["target_cls"].append(cls)
                    self.target_img.append(cls.unique())
                continue
            if single:
                pred[:, 5] = 0
            self.stats["tp"].append(tp_all[si, :npr])
            if tp_m_all is not None:
                self.stats[self.tp2_key].append(tp_m_all[si, :npr])
            self.stats["conf"].append(pred[:, 4])
            self.stats["pred_cls"].append(pred[:, 5])
            self.stats["target_cls"].append(cls)
            self.target_img.append(cls.unique())
            if save and self.args.get("save_json"):
                self.jdict.extend(self._json_rows(pred, si, im_files[si]))
            if save and self.args.get("save_txt"):
                self._save_txt(pred, si, ori_shapes[si], self.save_dir / "labels" / f"{Path(im_files[si]).stem}.txt")


class SegmentationValidator(DetectionValidator):
    """SegmentationValidator (U/models/yolo/segment/val.py): the detection validator plus the mask TP matrix
    ``stats["tp_m"]`` and SegmentMetrics.  Reached by Model.val when the model has a Segment head and ground-truth
    masks are supplied: tensor batches carry ``"masks"`` -- with overlap_mask=True (the default) the uint8 index map
    [B, gh, gw] in which value l + 1 marks the pixels of the image's l-th label (labels in the order the indices
    name, at most 255 per image), with overlap_mask=False planes [N, gh, gw] in label order; (gh, gw) normally a
    quarter of the image (mask_ratio 4).

    Per batch, right behind the box matching on the same stream and before the session runs again: the session's
    detections as bit planes at the image size (session.masks_bits = process_mask(upsample=True), val.py:93-97),
    the labels' masks resampled to that size as bit planes (ydbl_gt_mask_bits, val.py:204-212), their IoU by
    popcount (ydbl_mask_iou, val.py:213) and ydbl_match_iou (val.py:217).  Nothing of it is read back but the
    [B, max_det, n_iou] matrix, together with the box one.  The planes are addressed by slot (image b's at
    b * max_det), so no count is needed on the host before the launches; slots past an image's count are never
    written or read.  coco_eval, the confusion matrix, save_json / save_txt and loss stay box-based."""

    stat_keys = ("tp", "tp_m", "conf", "pred_cls", "target_cls")
    with_masks = True

    def __init__(self, model, args):
        super().__init__(model, args)
        self.metrics = SegmentMetrics(names=model.names)
        self.overlap = bool(args.get("overlap_mask", True))
        if args.get("save_json") or args.get("save_txt"):
            LOGGER.info("val() with mask metrics: save_json / save_txt write the box forms only (RLE needs "
                        "pycocotools, polygons need cv2)")

    def _launch(self, s, im, gt):
        self._sess = s  # the mask step reads its proto / coefficient buffers and det / count / keep_idx in place
        return super()._launch(s, im, gt)

    def _run_dataset(self, data, dev):
        if not self.overlap:
            raise ValueError("overlap_mask=False is for tensor batches: a dataset-backed val() builds the overlap "
                             "index map")
        super()._run_dataset(data, dev)

    def _run_tensor_batch(self, batch, dev):
        if "masks" not in batch:
            raise ValueError("val() with mask metrics: every batch must carry 'masks' (only some of them do)")
        self._gt_masks = batch["masks"]
        super()._run_tensor_batch(batch, dev)

    def _match_masks(self, det_d, cnt_d, grouped, bidx, single):
        from ..utils.ops import gt_mask_bits, mask_iou_bits

        s, dev = self._sess, det_d.device
        b, max_det = det_d.shape[0], det_d.shape[1]
        _, cls, ofs, n_gt = grouped
        m = torch.as_tensor(self._gt_masks)
        if m.dim() != 3:
            raise ValueError(f"'masks' must be [{'B' if self.overlap else 'N'}, gh, gw], got {tuple(m.shape)}")
        bidx = torch.as_tensor(bidx).reshape(-1).long()
        if self.overlap:
            if m.shape[0] != b:
                raise ValueError(f"overlap_mask=True: 'masks' is the index map [B, gh, gw]; got {m.shape[0]} maps for "
                                 f"{b} images")
            if n_gt and int(torch.bincount(bidx, minlength=b).max()) > 255:
                raise ValueError("overlap_mask=True: an index map names at most 255 labels per image")
        else:
            if m.shape[0] != n_gt:
                raise ValueError(f"overlap_mask=False: 'masks' holds one plane per label; got {m.shape[0]} for {n_gt}")
            m = m[torch.argsort(bidx, stable=True).to(m.device)]  # group_labels' order
        m = (m if self.overlap else m != 0).to(torch.uint8).to(dev).contiguous()
        words, _ = s.masks_bits([max_det] * b)
        gt_bits, area = gt_mask_bits(m, ofs, n_gt, (s.h, s.w), self.overlap)
        row = torch.arange(b, dtype=torch.int64, device=dev) * max_det
        iou = mask_iou_bits(words, row, cnt_d.to(torch.int32), max_det, gt_bits, ofs, area, (s.h, s.w))
        return match_iou_batch(det_d, cnt_d, iou, cls, ofs, self.iouv, single)

    def get_desc(self):
        """segment/val.py:53-69 with this fork's mAP75 column in both groups."""
        return ("%22s" + "%11s" * 12) % ("Class", "Images", "Instances", "Box(P", "R", "mAP50", "mAP75", "mAP50-95)",
                                         "Mask(P", "R", "mAP50", "mAP75", "mAP50-95)")


def gt_visibility(kpts: torch.Tensor) -> torch.Tensor:
    """Ground-truth keypoints [N, K, 2 or 3] as [N, K, 3]: two-column points get the reference's visibility column
    (U/data/utils.py:155-159: 0 where x or y is negative, else 1)."""
    if kpts.dim() != 3 or kpts.shape[-1] not in (2, 3):
        raise ValueError(f"'keypoints' must be [N, K, 2 or 3], got {tuple(kpts.shape)}")
    if kpts.shape[-1] == 3:
        return kpts
    vis = torch.where((kpts[..., 0] < 0) | (kpts[..., 1] < 0), 0.0, 1.0).to(kpts.dtype)
    return torch.cat([kpts, vis[..., None]], -1)


class PoseValidator(DetectionValidator):
    """PoseValidator (U/models/yolo/pose/val.py): the detection validator plus the keypoint TP matrix
    ``stats["tp_p"]`` and PoseMetrics.  Reached by Model.val when the model has a Pose head and ground-truth
    keypoints are supplied: tensor batches carry ``"keypoints"`` [N, K, 2 or 3] in label order, in the units of the
    batch's ``bboxes`` (pixels of the input image); a dataset's label rows have 5 + K * ndim columns.

    Per batch, right behind the box matching on the same stream and before the session runs again: the session's
    keypoints (written inside the graph by ydbl_pose_keypoints) and the labels' are brought to the space the boxes
    are matched in -- scale_coords: for tensor batches the clip to the input alone (gain 1, pad 0), for a dataset
    scale_coords(ratio_pad) to the native image (val.py:86-104) --, then ydbl_kpt_oks (the label areas from the label
    boxes, val.py:192) and ydbl_match_iou (val.py:197).  Nothing of it is read back but the [B, max_det, n_iou]
    matrix, together with the box one (and the keypoints themselves for save_json / save_txt).  coco_eval, the
    confusion matrix and loss stay box-based."""

    stat_keys = ("tp", "tp_p", "conf", "pred_cls", "target_cls")
    tp2_key = "tp_p"

    def __init__(self, model, args):
        super().__init__(model, args)
        self.metrics = PoseMetrics(names=model.names)
        self.kpt_shape = list(model.model.kpt_shape)
        K = self.kpt_shape[0]
        self.sigma = OKS_SIGMA if self.kpt_shape == [17, 3] else np.ones(K) / K  # val.py:77-84
        self._kpts_host = None

    def _launch(self, s, im, gt):
        self._sess = s  # the keypoint step reads its kpts in place
        return super()._launch(s, im, gt)

    def _dataset_kw(self) -> dict:
        return {"keypoints": True, "kpt_shape": self.kpt_shape}

    def _check_gt(self, kp):
        kp = gt_visibility(torch.as_tensor(kp).float())
        if kp.shape[1] != self.kpt_shape[0]:
            raise ValueError(f"'keypoints' holds {kp.shape[1]} points per label, the model {self.kpt_shape[0]}")
        return kp

    def _run_tensor_batch(self, batch, dev):
        from ..utils.ops import clip_coords

        if "keypoints" not in batch:
            raise ValueError("val() with keypoint metrics: every batch must carry 'keypoints' (only some of them do)")
        h, w = batch["img"].shape[-2:]
        self._gt_kpts = clip_coords(self._check_gt(batch["keypoints"]).clone(), (h, w))  # scale_coords: gain 1, pad 0
        self._pred_space = lambda kp: clip_coords(kp, (h, w))
        super()._run_tensor_batch(batch, dev)

    def _native_extra(self, hb, gain, pad, ori):
        """_prepare_batch / _prepare_pred (val.py:86-104) of one dataset batch: the labels' keypoints per image on the
        host in fp32 torch ops, as the reference runs them; the predictions' for the whole block on the device."""
        from ..utils.ops import scale_coords

        H, W = hb["shape"]
        kp = self._check_gt(hb["keypoints"]).clone()
        bidx = torch.from_numpy(hb["batch_idx"]).long()
        for si in range(len(hb["ori_shape"])):
            idx = bidx == si
            if idx.any():
                k = kp[idx]
                k[..., 0] *= W
                k[..., 1] *= H
                kp[idx] = scale_coords((H, W), k, hb["ori_shape"][si], ratio_pad=hb["ratio_pad"][si])
        self._gt_kpts = kp

        def pred_space(p):  # scale_coords(ratio_pad) + clip_coords on the padded [B, max_det, K, ndim] block
            p[..., 0:2] -= pad[:, None, None, :]
            p[..., 0:2] /= gain[:, None, None, None]
            p[..., 0:2] = torch.minimum(p[..., 0:2].clamp(min=0), ori[:, None, None, :])
            return p

        self._pred_space = pred_space

    def _match_masks(self, det_d, cnt_d, grouped, bidx, single):
        from ..utils.ops import kpt_oks

        dev = det_d.device
        boxes, cls, ofs, n_gt = grouped
        order = torch.argsort(torch.as_tensor(bidx).reshape(-1).long(), stable=True)  # group_labels' order
        if self._gt_kpts.shape[0] != n_gt:
            raise ValueError(f"'keypoints' holds {self._gt_kpts.shape[0]} labels, 'bboxes' {n_gt}")
        gt = self._gt_kpts[order].to(dev).contiguous()
        pred = self._pred_space(self._sess.kpts.clone())
        sigma = torch.as_tensor(np.asarray(self.sigma), dtype=torch.float32).to(dev)
        oks = kpt_oks(pred, cnt_d.to(torch.int32).contiguous(), gt, boxes, ofs, sigma)
        want = self.save_dir is not None and (self.args.get("save_json") or self.args.get("save_txt"))
        self._kpts_host = pred.cpu() if want else None
        return match_iou_batch(det_d, cnt_d, oks, cls, ofs, self.iouv, single)

    def _json_rows(self, pred, si, im_file) -> list:
        """pred_to_json (val.py:238-253): the rows gain "keypoints", the detection's K * ndim values."""
        rows = pred_to_json(pred, im_file)
        for r, k in zip(rows, self._kpts_host[si, : len(rows)].reshape(len(rows), -1).tolist()):
            r["keypoints"] = k
        return rows

    def _save_txt(self, pred, si, shape, file):
        """save_one_txt (val.py:226-236): the keypoints behind each box."""
        from .results import Results

        Results(None, path=None, names=self.model.names, boxes=pred[:, :6], orig_shape=(shape[0], shape[1]),
                keypoints=self._kpts_host[si, : len(pred)].clone()).save_txt(
                    file, save_conf=bool(self.args.get("save_conf", False)))

    def get_desc(self):
        """pose/val.py:47-62 with this fork's mAP75 column in both groups."""
        return ("%22s" + "%11s" * 12) % ("Class", "Images", "Instances", "Box(P", "R", "mAP50", "mAP75", "mAP50-95)",
                                         "Pose(P", "R", "mAP50", "mAP75", "mAP50-95)")


def pred_to_json(predn: torch.Tensor, filename, class_map=None) -> list:
    """pred_to_json (val.py:281-295): one COCO-format row per detection of one image.  A numeric stem becomes an
    int image_id; category_id = class_map[class] (default class + 1, val.py:77); bbox = top-left xywh rounded to
    3 places; score rounded to 5."""
    stem = Path(filename).stem
    image_id = int(stem) if stem.isnumeric() else stem
    box = torch.empty_like(predn[:, :4])  # xyxy2xywh (U/utils/ops.py:395-413), then centre -> top-left
    box[:, 0] = (predn[:, 0] + predn[:, 2]) / 2
    box[:, 1] = (predn[:, 1] + predn[:, 3]) / 2
    box[:, 2] = predn[:, 2] - predn[:, 0]
    box[:, 3] = predn[:, 3] - predn[:, 1]
    box[:, :2] -= box[:, 2:] / 2
    return [{"image_id": image_id, "category_id": class_map[int(p[5])] if class_map else int(p[5]) + 1,
             "bbox": [round(x, 3) for x in b], "score": round(p[4], 5)}
            for p, b in zip(predn.tolist(), box.tolist())]


def save_one_txt(predn: torch.Tensor, save_conf: bool, shape, names, file) -> None:
    """save_one_txt (val.py:270-279): 'cls xc yc w h [conf]' rows normalized by the original (h, w), appended."""
    from .results import Results

    Results(None, path=None, names=names, boxes=predn[:, :6], orig_shape=(shape[0], shape[1])).save_txt(
        file, save_conf=save_conf)


def native_labels(hb) -> torch.Tensor:
    """A host batch's labels (normalized xywh of the letterboxed image) -> xyxy in original-image pixels:
    DetectionValidator._prepare_batch (U/models/yolo/detect/val.py:104-115) with scale_boxes(ratio_pad)
    (U/utils/ops.py:92-127), per image as the reference runs it, in fp32 torch ops."""
    H, W = hb["shape"]
    boxes = torch.from_numpy(hb["bboxes"]).reshape(-1, 4)
    bidx = torch.from_numpy(hb["batch_idx"]).long()
    native = torch.zeros_like(boxes)
    for si in range(len(hb["ori_shape"])):
        idx = bidx == si
        if idx.any():
            bb = _xywh2xyxy(boxes[idx]) * torch.tensor((W, H, W, H))
            (g0, _), (pw, ph) = hb["ratio_pad"][si]
            bb[:, 0] -= pw
            bb[:, 1] -= ph
            bb[:, 2] -= pw
            bb[:, 3] -= ph
            bb /= g0
            h0, w0 = hb["ori_shape"][si]
            bb[:, 0].clamp_(0, w0)
            bb[:, 1].clamp_(0, h0)
            bb[:, 2].clamp_(0, w0)
            bb[:, 3].clamp_(0, h0)
            native[idx] = bb
    return native


def _has_images(p: Path) -> bool:
    from .dataset import IMG_FORMATS

    return any(f.suffix[1:].lower() in IMG_FORMATS for f in p.rglob("*.*"))


def _xywh2xyxy(x: torch.Tensor) -> torch.Tensor:
    """U/utils/ops.py:416-433."""
    y = torch.empty_like(x)
    xy, wh = x[..., :2], x[..., 2:] / 2
    y[..., :2] = xy - wh
    y[..., 2:] = xy + wh
    return y


def _scale_clip(boxes: torch.Tensor, pad: torch.Tensor, gain: torch.Tensor, wh: torch.Tensor) -> None:
    """scale_boxes(ratio_pad) + clip_boxes (U/utils/ops.py:92-127, :319-338) for a padded [B, max_det, 4] block
    of device boxes, in place; pad [B, 1, 2] (x, y), gain [B, 1, 1], wh [B, 1, 2] original (w, h)."""
    boxes[..., 0:2] -= pad
    boxes[..., 2:4] -= pad
    boxes /= gain
    boxes[..., 0:2] = torch.minimum(boxes[..., 0:2].clamp(min=0), wh)
    boxes[..., 2:4] = torch.minimum(boxes[..., 2:4].clamp(min=0), wh)
