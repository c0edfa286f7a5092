"""Per-image evaluation (COCO / ADE20k): semantic, panoptic and instance results of one image.

Counterpart of the reference's `InferenceImageGenericSegmentation` (univs/inference/inference_image_generic_seg.py):

    eval                   :173-205   normalise, LSJ square padding (or size_divisibility), targets ('detection': the class vocabulary
                                      of the dataset as text queries), the model at T = 1
    inference_image        :207-283   quality scores, stability filter, the three sub-tasks, the resize to the original size
    semantic_inference     :285-300
    panoptic_inference     :302-381
    instance_inference     :383-431
    postprocess_nms        :433-449   (torchvision's batched_nms: restated here, `batched_nms`)

What differs is where the work happens.  The reference resizes all Q' mask logits L [Q', h, w] to the padded input size (Hp, Wp) first
([333, 1024, 1024] fp32 = 1.4 GB at the shipped geometry) and then makes several full passes over that stack.  Here the HIP kernels of
csrc/image_post.hip read L and evaluate the resized values where they need them (ops.image_*); the stack is never built.  What stays in
PyTorch on the device is the glue on [Q', C]-sized tensors: sigmoid / softmax of the class logits, top-k, the thing filters and the IoU
matrix of the NMS.  The host reads the panoptic step's [K, 3] pixel counts once (the reference's own `.item()` calls, collapsed into one
transfer) and the NMS's [K, K] overlap flags.

Orders the reference leaves open (pinned here, tests compare as sets where they differ):
  * NMS visits boxes by descending score, equal scores by ascending index (torchvision's sort is not stable);
  * the instance top-k (`topk(sorted=False)`, :408) is returned by descending score, equal scores by ascending flat index.

On the CPU (and for shapes a kernel does not cover) the same steps run as their ATen formulation (`AtenSteps`): the reference's
expressions on the resized stack.
"""
from typing import Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import imagelabels_ops, ops
from ..registry import configurable
from ..utils.comm import convert_mask_to_box
from .results import rle_encode_masks
from .video_entity import COMBINED_DATASETS_CATEGORY_INFO, ImageList

SEMANTIC_TOPK = 200          # semantic_inference keeps the 200 best queries (:291)
OPEN_VOC_TEMPERATURE = 0.06  # softmax(cls / 0.06) "for open-voc settings" (:297, :315)
PANOPTIC_NMS_IOU = 0.9       # panoptic_inference's postprocess_nms (:311)
INSTANCE_NMS_IOU = 0.85      # postprocess_nms' default (:433)


class Boxes:
    """Minimal stand-in for detectron2.structures.Boxes: `.tensor` float32 [N, 4] XYXY."""

    def __init__(self, tensor):
        self.tensor = torch.as_tensor(tensor, dtype=torch.float32)

    def __len__(self):
        return int(self.tensor.shape[0])


class Instances:
    """Minimal stand-in for detectron2.structures.Instances: `image_size` (H, W) plus per-instance fields set as attributes."""

    def __init__(self, image_size, **fields):
        self.image_size = tuple(image_size)
        for k, v in fields.items():
            setattr(self, k, v)

    def __len__(self):
        return len(self.scores)


# ---- small host-side pieces ---------------------------------------------------------------------------------------------------------
def nms(boxes: torch.Tensor, scores: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """torchvision.ops.nms: greedy in descending score order, a box is suppressed when its IoU with a kept box is > iou_threshold;
    area = (x2 - x1) * (y2 - y1), IoU = inter / (area_i + area_j - inter) in fp32.  Equal scores: ascending index.  Returns the kept
    indices in visiting order.  The [K, K] overlaps are computed on the device of `boxes`, the greedy pass on the host."""
    n = int(boxes.shape[0])
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True)[1]
    b = boxes[order].float()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.maximum(b[:, None, :2], b[None, :, :2])
    rb = torch.minimum(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    over = (inter / (area[:, None] + area[None, :] - inter) > iou_threshold).cpu().numpy()
    suppressed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if suppressed[i]:
            continue
        keep.append(i)
        suppressed |= over[i]
    return order[torch.as_tensor(keep, dtype=torch.int64, device=boxes.device)]


def batched_nms(boxes: torch.Tensor, scores: torch.Tensor, idxs: torch.Tensor, iou_threshold: float) -> torch.Tensor:
    """torchvision.ops.batched_nms (coordinate trick): boxes of different categories are moved apart by idx * (max coordinate + 1) so that
    they never overlap, then one `nms`."""
    if boxes.numel() == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    max_coordinate = boxes.max()
    offsets = idxs.to(boxes) * (max_coordinate + torch.tensor(1).to(boxes))
    return nms(boxes + offsets[:, None], scores, iou_threshold)


def panoptic_segments(counts, classes, thing_ids, overlap_threshold):
    """The segment loop of panoptic_inference (:338-379) on the per-k pixel counts [K, 3] = (|ids == k|, |sigmoid(U_k) >= 0.5|,
    |ids == k and covered|) and the kept classes [K]: returns (lut [K] int, segments_info).  lut[k] is the segment id painted where k
    won and is covered (0: not painted); stuff classes seen again are merged into their first segment."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
    classes = [int(c) for c in classes]
    lut = [0] * len(classes)
    segments_info = []
    stuff_memory = {}
    current_segment_id = 0
    for k, pred_class in enumerate(classes):
        isthing = pred_class in thing_ids
        mask_area, original_area, both = (int(v) for v in counts[k])
        if mask_area > 0 and original_area > 0 and both > 0:
            if mask_area / original_area < overlap_threshold:
                continue
            if not isthing:
                if pred_class in stuff_memory:
                    lut[k] = stuff_memory[pred_class]
                    continue
                stuff_memory[pred_class] = current_segment_id + 1
            current_segment_id += 1
            lut[k] = current_segment_id
            segments_info.append({"id": current_segment_id, "isthing": bool(isthing), "category_id": pred_class})
    return lut, segments_info


def fused_or_aten(r, aten, *args):
    """The result `r` of a fused step (ops.image_* / ops.video_*), or `aten(*args)` where its kernel does not cover the call (None)."""
    return aten(*args) if r is None else r


def nearest_source_index(dst, in_size: int, out_size: int):
    """ATen's nearest source index (UpSampleNearest2d.cu): min(floor(dst * (in / out)), in - 1), the scale and the product in fp32."""
    scale = np.float32(in_size) / np.float32(out_size)
    d = np.asarray(dst, dtype=np.float32)
    return np.minimum(np.floor(d * scale).astype(np.int64), in_size - 1)


def _record(hi, lo, box, nonempty):
    z = torch.zeros_like(hi)
    return torch.stack([hi, lo, box[:, 0], box[:, 1], box[:, 2], box[:, 3], nonempty, z], -1).to(torch.int32)


class AtenSteps:
    """The ATen formulation of every kernel of csrc/image_post.hip: the reference's expressions on the resized stack U = bilinear(L ->
    padded), made once.  The CPU path of the driver, the fall-back for shapes a kernel does not cover, and the yardstick of the tests and
    of tools/image_bench.py."""

    def __init__(self, L, padded, crop):
        self.L, self.padded, self.crop = L, tuple(int(v) for v in padded), tuple(int(v) for v in crop)
        self._U = None

    @property
    def U(self):
        if self._U is None:
            self._U = F.interpolate(self.L[None], size=self.padded, mode="bilinear", align_corners=False)[0]
        return self._U

    def cropped(self, planes):
        hi, wi = self.crop
        return self.U[planes.long(), :hi, :wi]

    def mask_stats(self):
        hi, wi = self.crop
        U = self.U
        c = U[:, :hi, :wi] > 0
        box = convert_mask_to_box(c).long()
        return _record((U > 1).flatten(1).sum(-1), (U > -1).flatten(1).sum(-1), box, c.flatten(1).any(-1).long())

    def panoptic_ids(self, planes, scores):
        m = self.cropped(planes).sigmoid()
        ids = (scores.view(-1, 1, 1) * m).argmax(0)
        cov = m.gather(0, ids[None])[0] >= 0.5
        K = int(planes.numel())
        counts = torch.stack([torch.bincount(ids.flatten(), minlength=K), (m >= 0.5).flatten(1).sum(-1),
                              torch.bincount(ids[cov], minlength=K)], -1)
        return (ids | (cov.to(ids.dtype) << 30)).to(torch.int32), counts.to(torch.int32)

    @staticmethod
    def panoptic_paint(ids, lut, out_size):
        lut = torch.as_tensor(lut, dtype=torch.int32, device=ids.device)
        k = (ids & ((1 << 30) - 1)).long()
        val = torch.where((ids & (1 << 30)) != 0, lut[k], torch.zeros_like(ids))
        out = F.interpolate(val[None, None].float(), size=tuple(out_size), mode="nearest")[0, 0].to(torch.int32)
        present = torch.unique(out)
        seen = ((lut != 0) & torch.isin(lut, present)).to(torch.int32)
        return out, seen

    def semseg(self, planes, probs):
        return torch.einsum("qc,qhw->chw", probs, self.cropped(planes).sigmoid())

    @staticmethod
    def semseg_labels(r, out_size):
        """argmax(0) of the resized semantic result as uint8 [H, W]: what an evaluator makes of `sem_seg` first.  The resize is the one
        the "scores" result goes through (`_resize_bilinear`: F.interpolate on the CPU), so the labels are the argmax of those scores."""
        return _resize_bilinear(r, out_size).argmax(0).to(torch.uint8)

    def instance_masks(self, planes, out_size):
        m = self.cropped(planes)
        if tuple(m.shape[-2:]) != tuple(out_size):
            m = F.interpolate(m[None], size=tuple(out_size), mode="bilinear", align_corners=False)[0]
        b = m > 0
        box = convert_mask_to_box(b).long() if b.numel() else torch.zeros((0, 4), dtype=torch.long, device=b.device)
        z = torch.zeros(b.shape[0], dtype=torch.long, device=b.device)
        return b.to(torch.uint8), _record(z, z, box, b.flatten(1).any(-1).long() if b.numel() else z)


class FusedSteps:
    """The same steps on csrc/image_post.hip (ops.image_*); each falls back to `AtenSteps` only where its kernel does not cover the shape
    (the ops return None there: grid / LDS limits)."""

    def __init__(self, L, padded, crop):
        self.L, self.padded, self.crop = L.contiguous(), tuple(int(v) for v in padded), tuple(int(v) for v in crop)
        self.aten = AtenSteps(self.L, padded, crop)

    def mask_stats(self):
        return fused_or_aten(ops.image_mask_stats(self.L, self.padded, self.crop), self.aten.mask_stats)

    def panoptic_ids(self, planes, scores):
        return fused_or_aten(ops.image_panoptic_ids(self.L, self.padded, self.crop, planes, scores), self.aten.panoptic_ids, planes, scores)

    def panoptic_paint(self, ids, lut, out_size):
        r = ops.image_panoptic_paint(ids, torch.as_tensor(lut, dtype=torch.int32, device=ids.device), out_size)
        return fused_or_aten(r, AtenSteps.panoptic_paint, ids, lut, out_size)

    def semseg(self, planes, probs):
        return fused_or_aten(ops.image_semseg(self.L, self.padded, self.crop, planes, probs), self.aten.semseg, planes, probs)

    @staticmethod
    def semseg_labels(r, out_size):
        r = r.contiguous()
        return fused_or_aten(imagelabels_ops.semseg_labels(r, out_size), AtenSteps.semseg_labels, r, out_size)

    def instance_masks(self, planes, out_size):
        r = ops.image_instance_masks(self.L, self.padded, self.crop, planes, out_size)
        return fused_or_aten(r, self.aten.instance_masks, planes, out_size)


def _resize_bilinear(x, size):
    if x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled():
        return ops.bilinear_resample(x, size)
    return F.interpolate(x[None], size=tuple(size), mode="bilinear", align_corners=False)[0]


class InferenceImageGenericSegmentation(nn.Module):
    @configurable
    def __init__(
        self,
        *,
        num_queries: int,
        object_mask_threshold: float,
        overlap_threshold: float,
        stability_score_thresh: float,
        size_divisibility: int,
        LSJ_aug_image_size: int,
        LSJ_aug_enable_test: bool,
        sem_seg_postprocess_before_inference: bool,
        pixel_mean: Tuple[float],
        pixel_std: Tuple[float],
        prompt_as_queries: bool,
        semantic_on: bool,
        instance_on: bool,
        panoptic_on: bool,
        disable_semantic_queries: bool,
        test_topk_per_image: int,
        thing_contiguous_ids=(),
        dataset_category_info=None,
        fused: bool = True,
        sem_seg_as: str = "scores",
    ):
        """`thing_contiguous_ids`: the contiguous category indices that are things, in the order of the reference's
        `metadata.thing_dataset_id_to_contiguous_id.values()` (the instance sub-task keeps those class columns in that order) -- one
        sequence for every dataset, or a mapping {dataset name: sequence} (COCO panoptic and ADE20k have different vocabularies).  The
        panoptic and instance sub-tasks refuse to run without them: with none, every thing class would silently be treated as stuff.
        `fused=False` runs the ATen formulation of every step on the device (tools/image_bench.py's yardstick).
        `sem_seg_as` (an attribute, may be set after construction): "scores" returns the semantic result as `sem_seg`, float32 [C, H, W];
        "labels" returns `sem_seg_labels`, uint8 [H, W] = its argmax(0), instead, without building the [C, H, W] tensor."""
        super().__init__()
        self.num_queries = num_queries
        self.object_mask_threshold = object_mask_threshold
        self.overlap_threshold = overlap_threshold
        self.stability_score_thresh = stability_score_thresh
        self.size_divisibility = size_divisibility
        self.LSJ_aug_image_size = LSJ_aug_image_size
        self.LSJ_aug_enable_test = LSJ_aug_enable_test
        self.sem_seg_postprocess_before_inference = sem_seg_postprocess_before_inference
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(-1, 1, 1), False)
        self.prompt_as_queries = prompt_as_queries
        self.semantic_on = semantic_on
        self.instance_on = instance_on
        self.panoptic_on = panoptic_on
        self.disable_semantic_queries = disable_semantic_queries
        self.test_topk_per_image = test_topk_per_image
        self.thing_contiguous_ids = ({str(k): [int(c) for c in v] for k, v in thing_contiguous_ids.items()}
                                     if isinstance(thing_contiguous_ids, dict) else [int(c) for c in thing_contiguous_ids])
        self.dataset_category_info = COMBINED_DATASETS_CATEGORY_INFO if dataset_category_info is None else dataset_category_info
        self.fused = fused
        self.sem_seg_as = sem_seg_as

    @classmethod
    def from_config(cls, cfg, thing_contiguous_ids=(), dataset_category_info=None):
        t = cfg.MODEL.MASK_FORMER.TEST
        return {
            "num_queries": cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES,
            "object_mask_threshold": t.OBJECT_MASK_THRESHOLD,
            "overlap_threshold": t.OVERLAP_THRESHOLD,
            "stability_score_thresh": t.STABILITY_SCORE_THRESH,
            "size_divisibility": cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY,
            "LSJ_aug_image_size": cfg.INPUT.LSJ_AUG.IMAGE_SIZE,
            "LSJ_aug_enable_test": cfg.INPUT.LSJ_AUG.SQUARE_ENABLED,
            "sem_seg_postprocess_before_inference": t.SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE,
            "pixel_mean": cfg.MODEL.PIXEL_MEAN,
            "pixel_std": cfg.MODEL.PIXEL_STD,
            "prompt_as_queries": cfg.MODEL.UniVS.PROMPT_AS_QUERIES,
            "semantic_on": t.SEMANTIC_ON,
            "instance_on": t.INSTANCE_ON,
            "panoptic_on": t.PANOPTIC_ON,
            "disable_semantic_queries": cfg.MODEL.UniVS.TEST.DISABLE_SEMANTIC_QUERIES,
            "test_topk_per_image": cfg.TEST.DETECTIONS_PER_IMAGE,
            "thing_contiguous_ids": thing_contiguous_ids,
            "dataset_category_info": dataset_category_info,
        }

    @property
    def device(self):
        return self.pixel_mean.device

    # ---- entry point -------------------------------------------------------------------------------------------------------------
    def things(self, dataset_name=None):
        ids = self.thing_contiguous_ids
        if isinstance(ids, dict):
            ids = ids.get(dataset_name, ())
        return [int(c) for c in ids]

    def check_things(self, dataset_name):
        if (self.panoptic_on or self.instance_on) and not self.things(dataset_name):
            raise ValueError(f"panoptic / instance inference on {dataset_name!r} needs the thing categories: set "
                             "thing_contiguous_ids (the reference reads them from metadata.thing_dataset_id_to_contiguous_id)")

    def check_dataset(self, dataset_name):
        """Image datasets are named by their class vocabulary (the reference's mapper: 'coco_panoptic', 'coco', 'ade20k';
        univs/data/dataset_mapper.py:465-468); any other name has no vocabulary to score against."""
        if dataset_name not in self.dataset_category_info:
            raise NotImplementedError(
                f"per-image evaluation of {dataset_name!r}: no class vocabulary of that name (image datasets are named after theirs: "
                f"'coco_panoptic', 'coco', 'ade20k')")
        if not (dataset_name.startswith("coco") or dataset_name.startswith("ade20k")
                or dataset_name in getattr(self, "installed_vocabularies", ())):          # (vocabulary.install)
            raise ValueError(f"do not support the model inference on {dataset_name}.")
        if self.sem_seg_postprocess_before_inference:
            raise NotImplementedError("MODEL.MASK_FORMER.TEST.SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE True is not built")
        self.check_things(dataset_name)

    def padded_size(self, sizes):
        d = self.size_divisibility
        if self.LSJ_aug_enable_test:
            H = W = int(self.LSJ_aug_image_size)
            if max(s[0] for s in sizes) > H or max(s[1] for s in sizes) > W:
                raise ValueError(f"image of size {sizes} larger than the LSJ square {H}")
        else:
            H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
        if d > 1:
            H, W = (H + d - 1) // d * d, (W + d - 1) // d * d
        return H, W

    def image_list(self, frames):
        sizes = [tuple(int(v) for v in f.shape[-2:]) for f in frames]
        Hp, Wp = self.padded_size(sizes)
        if frames[0].is_cuda and frames[0].dtype == torch.float32 and all(f.shape == frames[0].shape for f in frames):
            out = ops.normalize_pad(torch.stack(frames), self.pixel_mean, self.pixel_std, pad_to=(Hp, Wp))
            if out is not None:
                return ImageList(out, sizes)
        out = frames[0].new_zeros((len(frames), frames[0].shape[0], Hp, Wp), dtype=torch.float32)
        for i, f in enumerate(frames):
            out[i, :, : f.shape[-2], : f.shape[-1]] = (f.float() - self.pixel_mean) / self.pixel_std
        return ImageList(out, sizes)

    @torch.no_grad()
    def eval(self, model, batched_inputs):
        """batched_inputs: the mapper's per-image dicts {"image": [CHW tensor 0..255], "height", "width", "dataset_name", "task",
        "file_names", ...}; one result dict per image."""
        self.check_dataset(batched_inputs[0]["dataset_name"])
        frames = [f.to(self.device).float() for item in batched_inputs for f in item["image"]]
        images = self.image_list(frames)
        targets = model.prepare_targets.process_inference(batched_inputs, tuple(images.tensor.shape[-2:]), self.device,
                                                          getattr(model, "text_prompt_encoder", None), images.image_sizes[0])
        return self.inference_image(model, batched_inputs, images, targets)

    def inference_image(self, model, batched_inputs, images, targets):
        features = model.backbone(images.tensor)
        outputs = model.sem_seg_head(features, targets=targets)
        name = batched_inputs[0]["dataset_name"]
        num_classes, start = self.dataset_category_info[name]
        cls = outputs["pred_logits"][..., start:start + num_classes]
        masks = outputs["pred_masks"][:, :, 0]
        padded = tuple(images.tensor.shape[-2:])
        results = []
        for b, (item, image_size) in enumerate(zip(batched_inputs, images.image_sizes)):
            out_size = (int(item.get("height", image_size[0])), int(item.get("width", image_size[1])))
            results.append(self.postprocess(cls[b], masks[b], padded, image_size, out_size, dataset_name=name))
        return results

    # ---- post-processing of one image --------------------------------------------------------------------------------------------
    def postprocess(self, cls_logits, mask_logits, padded, image_size, out_size, dataset_name=None):
        """cls_logits [Q', C] (the dataset's columns, before the sigmoid), mask_logits L [Q', h, w] -> {"sem_seg" (or "sem_seg_labels":
        `sem_seg_as`), "panoptic_seg", "instances", "instances_rle"} as enabled (:226-283).  `dataset_name` selects the thing categories when they are a mapping."""
        self.check_things(dataset_name)
        things = self.things(dataset_name)
        image_size = tuple(int(v) for v in image_size)
        out_size = tuple(int(v) for v in out_size)
        L = mask_logits.float()
        steps = FusedSteps(L, padded, image_size) if (self.fused and L.is_cuda) else AtenSteps(L, padded, image_size)
        st = steps.mask_stats()
        scores_mask = st[:, 0].float() / st[:, 1].clamp(min=1).float()
        mask_cls = cls_logits.float().sigmoid() * scores_mask.unsqueeze(-1)
        rows = torch.arange(L.shape[0], device=L.device)          # the plane of L behind each row
        boxes = st[:, 2:6].long()                                 # convert_mask_to_box(crop(U) > 0)
        if self.stability_score_thresh > 0:
            keep = scores_mask > self.stability_score_thresh
            mask_cls, rows, boxes = mask_cls[keep], rows[keep], boxes[keep]
        result = {}
        if self.sem_seg_as not in ("scores", "labels"):
            raise ValueError(f"sem_seg_as={self.sem_seg_as!r}: 'scores' or 'labels'")
        if self.semantic_on:
            key = "sem_seg" if self.sem_seg_as == "scores" else "sem_seg_labels"
            result[key] = self.semantic_inference(steps, mask_cls, rows, out_size)
        if self.panoptic_on:
            result["panoptic_seg"] = self.panoptic_inference(steps, mask_cls, rows, boxes, out_size, things)
        if self.instance_on:
            inst = self.instance_inference(steps, mask_cls, rows, boxes, out_size, things)
            result["instances"] = inst
            result["instances_rle"] = rle_encode_masks(inst.pred_masks_u8)
        return result

    def semantic_inference(self, steps, mask_cls, rows, out_size):
        if self.prompt_as_queries and self.disable_semantic_queries:
            mask_cls, rows = mask_cls[self.num_queries:], rows[self.num_queries:]
        # (k = 200 in the reference, which raises with fewer rows; the same selection wherever it does not)
        top = torch.topk(mask_cls.max(-1)[0], k=min(SEMANTIC_TOPK, mask_cls.shape[0]))[1]
        probs = (mask_cls[top] / OPEN_VOC_TEMPERATURE).softmax(-1)
        r = steps.semseg(rows[top], probs)
        if self.sem_seg_as == "labels":
            return steps.semseg_labels(r, out_size)              # argmax(0) of the resize below, which is not built
        out = _resize_bilinear(r, out_size)                      # sem_seg_postprocess: the crop is already r's extent
        del r
        return out

    def panoptic_inference(self, steps, mask_cls, rows, boxes, out_size, things):
        if self.prompt_as_queries:
            pos = torch.arange(mask_cls.shape[0], device=mask_cls.device)
            thing_t = torch.as_tensor(things, dtype=torch.long, device=mask_cls.device)
            sel = (pos < self.num_queries) | ~torch.isin(pos - self.num_queries, thing_t)
            mask_cls, rows, boxes = mask_cls[sel], rows[sel], boxes[sel]
        s, lab = mask_cls.max(-1)
        keep = batched_nms(boxes.float(), s, lab, PANOPTIC_NMS_IOU)
        mask_cls, rows = mask_cls[keep], rows[keep]
        scores, _ = mask_cls.max(-1)
        keep = scores > self.object_mask_threshold
        scores, labels = (mask_cls / OPEN_VOC_TEMPERATURE).softmax(-1).max(-1)
        cur_scores, cur_classes, cur_rows = scores[keep], labels[keep], rows[keep]
        if cur_rows.numel() == 0:
            return torch.zeros(out_size, dtype=torch.int32, device=mask_cls.device), []
        ids, counts = steps.panoptic_ids(cur_rows, cur_scores)
        host = torch.cat([counts.long().flatten(), cur_classes.long()]).cpu().numpy()   # the one read-back of the step
        K = cur_rows.numel()
        lut, segments_info = panoptic_segments(host[: 3 * K].reshape(K, 3), host[3 * K:], set(things),
                                               self.overlap_threshold)
        pan, seen = steps.panoptic_paint(ids, lut, out_size)
        seen = seen.cpu().numpy()
        present = {lut[k] for k in range(K) if seen[k]}
        return pan, [info for info in segments_info if info["id"] in present]

    def instance_inference(self, steps, mask_cls, rows, boxes, out_size, things):
        if self.prompt_as_queries:
            mask_cls, rows, boxes = mask_cls[: self.num_queries], rows[: self.num_queries], boxes[: self.num_queries]
        if len(things) != mask_cls.shape[-1]:
            labels = mask_cls.max(-1)[1]
            cols = torch.as_tensor(things, dtype=torch.long, device=mask_cls.device)
            mask_cls = mask_cls[:, cols]
            keep = torch.isin(labels, cols)
            if int(keep.sum()) == 0:
                s = mask_cls.max(-1)[0]
                keep = s >= min(0.1, float(s.max()))
            mask_cls, rows, boxes = mask_cls[keep], rows[keep], boxes[keep]
        s, lab = mask_cls.max(-1) if mask_cls.numel() else (mask_cls.new_zeros(0), mask_cls.new_zeros(0, dtype=torch.long))
        keep = batched_nms(boxes.float(), s, lab, INSTANCE_NMS_IOU)
        mask_cls, rows = mask_cls[keep], rows[keep]
        C = mask_cls.shape[-1]
        flat = mask_cls.flatten()
        k = min(self.test_topk_per_image, flat.numel())
        order = torch.sort(flat, descending=True, stable=True)[1][:k]    # topk: descending score, ties by ascending flat index
        scores, labels = flat[order], order % C
        qrows = rows[torch.div(order, C, rounding_mode="floor")]
        masks, rec = steps.instance_masks(qrows, out_size)
        inst = Instances(out_size, pred_masks=masks.float(), pred_boxes=Boxes(rec[:, 2:6]), scores=scores, pred_classes=labels)
        inst.pred_masks_u8 = masks
        return inst
