"""MinVIS-style video inference of the non-unified configs (MODEL.UniVS.TEST.VIDEO_UNIFIED_INFERENCE_ENABLE False): VIS on 'ytvis*' /
'ovis*' and online VPS on 'vipseg*'.

Counterparts of the reference's two drivers:

    InferenceVideoVISFast   univs/inference/inference_video_vis_fast.py
        eval                                    :184-217   normalise, pad, targets, 'minvis' only
        inference_video_vis_minvis              :219-297   the stride-1 clip loop (run_minvis_loop)
        inference_video_vis_minvis_save_video   :299-351   top-k rows, flat (row, class) top-k, quality scores, masks
    InferenceVideoVPS       univs/inference/inference_video_vps.py
        eval                                    :175-204
        inference_video_vps_online              :206-293   the same loop, its own matching (match_from_embds :295-307)
        inference_video_vps_save_results        :309-406   keep rule, argmax map, per-segment areas, stuff merging, painting

The clip loop.  Clips run at stride 1; each clip's queries are Hungarian-matched to the embeddings of the previous two clips.  The
reference keeps every clip's [Q', T, h, w] mask logits in a list and averages each frame over the clips that cover it at the end.  Here
the matched masks go into one running sum S [Q', V, h, w] fp32 (V = video length), allocated once (ops.minvis_accumulate on the GPU),
and S is scaled in place to the per-frame mean as ATen's `mean` rounds: on the GPU a product with the factor 1 / n_v (MeanOps), on the
CPU a division by n_v (sum, then div_).  At T = 2 (every shipped config) each frame has at most two terms and the mean is the
reference's bit for bit; at T >= 3 only the order of the summation differs (clips are added in order, the reference's stack starts
with the newest clip).

Post-processing.  The reference then resizes all selected masks of all frames to the padded size ([K, V, Hp, Wp] fp32).  Here the HIP
kernels of csrc/video_post.hip read the mean and evaluate the resized values where they need them (`FusedSteps`); the stack is never
built.  On the CPU (and where a kernel does not cover the shape) the same steps run as their ATen formulation (`AtenSteps`): the
reference's expressions on the resized stack.

Orders the reference leaves open (tests compare as sets where they differ):
  * the VIS records (`topk(sorted=False)`, :321) are returned by descending final score (after the quality factor), equal scores by
    ascending flat (row, class) index; a row can appear more than once, with different labels, and shares its mask tensor between
    those records.

Settings: MERGE_ON_CPU is accepted and has no effect -- its purpose, bounding device memory, is served by the running sum.  The drivers
run on one GPU: they raise if a frame shard is set.  TRACKER_TYPE 'mdqe' (the MDQE over-tracker) is not built.
"""
from typing import Tuple

import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment
from torch import nn

from .. import ops
from ..registry import configurable
from ..utils.comm import calculate_mask_quality_scores
from .comm import match_from_learnable_embds
from .image_generic_seg import InferenceImageGenericSegmentation, fused_or_aten, panoptic_segments
from .results import rle_encode_masks
from .video_entity import COMBINED_DATASETS_CATEGORY_INFO

FIRST_CLIP_MAX_QUERIES = 100   # the first clip keeps the top min(Q, 100) of all queries (vis_fast :246, vps :233)
VPS_QUALITY_STEP = 5           # calculate_mask_quality_scores(cur_masks[:, ::5]) (vps :346)


def match_from_embds(tgt_embds, cur_embds):
    """The VPS driver's matching (inference_video_vps.py:295-307): cosine similarity, Hungarian assignment on the transposed cost;
    returns the permutation that aligns the current rows to the targets."""
    cur = cur_embds / cur_embds.norm(dim=1)[:, None]
    tgt = tgt_embds / tgt_embds.norm(dim=1)[:, None]
    cost = (1 - torch.mm(cur, tgt.transpose(0, 1))).cpu()
    return linear_sum_assignment(cost.transpose(0, 1))[1]


def clip_frame_counts(n_clips, T):
    """n_v: the number of clips covering frame v of a video of n_clips + T - 1 frames (stride 1)."""
    V = n_clips + T - 1
    return [sum(1 for t in range(min(v + 1, T)) if v - t < n_clips) for v in range(V)]


def scale_to_mean_(S, counts):
    """S [Q', V, h, w] sum over n_v clips -> the mean, in place, rounded as ATen's mean of the stacked terms: on the GPU
    sum * (1 / n_v) with the factor in fp32 (MeanOps), on the CPU sum / n_v (mean_out: sum then div_)."""
    n = torch.tensor(counts, dtype=torch.float32).view(1, -1, 1, 1)
    if S.is_cuda:
        return S.mul_((1.0 / n).to(S.device))
    return S.div_(n)


def run_minvis_loop(model, images, targets, *, num_frames, window, num_queries, stability_score_thresh, vps_matching, fused=True):
    """The stride-1 clip loop of both drivers (vis_fast :219-297, vps :206-293) -> (mean class logits [Q', C_all], mean mask logits
    [Q', V, h, w]).  `vps_matching` selects the VPS driver's embedding memory and matching (match_from_embds on clip-mean embeddings)
    instead of the VIS driver's (match_from_learnable_embds on the previous two clips' embeddings against the clip's [Q, T, C])."""
    x = images.tensor
    V, T = int(x.shape[0]), int(num_frames)
    if V < T:
        raise ValueError(f"a video of {V} frames is shorter than one clip (INPUT.SAMPLING_FRAME_NUM = {T})")
    n_clips = V - T + 1
    use_kernel = fused and x.is_cuda
    S = logit_sum = feats_w = None
    mem = []
    start, end = 0, 0
    for i in range(n_clips):
        targets[0]["frame_indices"] = torch.arange(i, i + T)
        if i + T > end:
            start, end = i, i + window
            feats_w = model.backbone(x[start:end])
        features = {k: v[i - start:i - start + T] for k, v in feats_w.items()}
        out = model.sem_seg_head(features, targets=targets)
        logits, masks, embds = out["pred_logits"][0], out["pred_masks"][0], out["pred_embds"][0]
        if i == 0:
            s = logits.sigmoid()
            if stability_score_thresh > 0:
                s = s + calculate_mask_quality_scores(masks).view(-1, 1)
            perm = torch.sort(s.max(-1)[0], descending=True)[1][:min(num_queries, FIRST_CLIP_MAX_QUERIES)][:num_queries]
            cur = embds[perm].float()
            mem.append(cur.mean(1))
        else:
            cur = embds[:num_queries].float()
            if vps_matching:
                cur = cur.mean(1)
                idx = match_from_embds(torch.stack(mem[-2:]).mean(dim=0), cur)
                mem.append(cur[idx])
            else:
                idx = match_from_learnable_embds(torch.stack(mem[-2:], dim=1), cur)
                mem.append(cur[idx].mean(1))
            perm = torch.as_tensor(np.asarray(idx), dtype=torch.int64, device=logits.device)
        mem = mem[-2:]
        lg = logits[perm].float()
        logit_sum = lg if logit_sum is None else logit_sum + lg      # sum(out_logits): the same order of additions
        if S is None:
            S = torch.zeros((int(perm.numel()), V) + tuple(masks.shape[-2:]), dtype=torch.float32, device=masks.device)
        if use_kernel:
            ops.minvis_accumulate(S, masks.float(), perm, i)
        else:
            S[:, i:i + T] += masks[perm].float()
        del out, masks
    return logit_sum / n_clips, scale_to_mean_(S, clip_frame_counts(n_clips, T))


# ---- the post-processing steps ------------------------------------------------------------------------------------------------------
class AtenSteps:
    """The ATen formulation of every kernel of csrc/video_post.hip: the reference's expressions on the resized stack U = bilinear(M ->
    padded), cropped.  The CPU path of the drivers, the fall-back for shapes a kernel does not cover, and the yardstick of the tests and
    of tools/minvis_bench.py."""

    def __init__(self, M, padded, crop):
        self.M, self.padded, self.crop = M, tuple(int(v) for v in padded), tuple(int(v) for v in crop)
        self._P = None

    def U(self, rows):
        hi, wi = self.crop
        return F.interpolate(self.M[rows.long()], size=self.padded, mode="bilinear", align_corners=False)[:, :, :hi, :wi]

    def mask_stats(self, rows, step):
        U = self.U(rows)[:, ::step]
        return torch.stack([(U > 1).flatten(1).sum(-1), (U > -1).flatten(1).sum(-1)], -1).to(torch.int32)

    def instance_masks(self, rows, out_size):
        U = self.U(rows)
        return torch.stack([F.interpolate(m[None], size=tuple(out_size), mode="bilinear", align_corners=False)[0] > 0
                            for m in U]).to(torch.uint8)

    def probs(self, rows):
        if self._P is None:
            self._P = self.U(rows).sigmoid()
        return self._P

    def panoptic_ids(self, rows, scores):
        P = self.probs(rows)
        is_bg = (P < 0.5).sum(0) == len(P)
        ids = (scores.view(-1, 1, 1, 1).to(P) * P).argmax(0)
        ids[is_bg] = -1
        return ids.to(torch.int32)

    def _ids_out(self, ids, out_size):
        return F.interpolate(ids.float().unsqueeze(0), size=tuple(out_size), mode="nearest").long().squeeze(0)

    def panoptic_counts(self, rows, ids, out_size):
        P, ido = self.probs(rows), self._ids_out(ids, out_size)
        counts = []
        for k in range(len(P)):
            pk = F.interpolate(P[k].unsqueeze(0), size=tuple(out_size), mode="bilinear", align_corners=False).squeeze(0) >= 0.5
            counts.append([int((ido == k).sum()), int(pk.sum()), int(((ido == k) & pk).sum())])
        return torch.tensor(counts, dtype=torch.int32).view(-1, 3)

    def panoptic_paint(self, rows, ids, lut, out_size):
        P, ido = self.probs(rows), self._ids_out(ids, out_size)
        out = torch.zeros(ido.shape, dtype=torch.int32, device=ido.device)
        for k, v in enumerate(lut):
            if v:
                pk = F.interpolate(P[k].unsqueeze(0), size=tuple(out_size), mode="bilinear", align_corners=False).squeeze(0) >= 0.5
                out[(ido == k) & pk] = int(v)
        return out


class FusedSteps:
    """The same steps on csrc/video_post.hip (ops.video_*); each falls back to `AtenSteps` only where its kernel does not cover the shape
    (the ops return None there)."""

    def __init__(self, M, padded, crop):
        self.M, self.padded, self.crop = M.contiguous(), tuple(int(v) for v in padded), tuple(int(v) for v in crop)
        self.aten = AtenSteps(self.M, padded, crop)

    def mask_stats(self, rows, step):
        return fused_or_aten(ops.video_mask_stats(self.M, self.padded, self.crop, rows, step), self.aten.mask_stats, rows, step)

    def instance_masks(self, rows, out_size):
        r = ops.video_instance_masks(self.M, self.padded, self.crop, rows, out_size)
        return fused_or_aten(r, self.aten.instance_masks, rows, out_size)

    def panoptic_ids(self, rows, scores):
        return fused_or_aten(ops.video_panoptic_ids(self.M, self.padded, self.crop, rows, scores), self.aten.panoptic_ids, rows, scores)

    def panoptic_counts(self, rows, ids, out_size):
        r = ops.video_panoptic_counts(self.M, self.padded, self.crop, rows, ids, out_size)
        return fused_or_aten(r, self.aten.panoptic_counts, rows, ids, out_size)

    def panoptic_paint(self, rows, ids, lut, out_size):
        r = ops.video_panoptic_paint(self.M, self.padded, self.crop, rows, ids, torch.as_tensor(lut, dtype=torch.int32), out_size)
        return fused_or_aten(r, self.aten.panoptic_paint, rows, ids, lut, out_size)


def _masks_to_host(steps, rows, out_size):
    """bool CPU [V, H0, W0] per row of `rows` (distinct).  On the GPU one kernel per row, its copy to pinned host memory on a side stream:
    the copy of row r overlaps the kernel of row r + 1, and the device holds about two rows' masks at a time."""
    M = steps.M
    if not M.is_cuda:
        return [m.bool() for m in steps.instance_masks(rows, out_size)]
    V = int(M.shape[1])
    side = torch.cuda.Stream(device=M.device)
    main = torch.cuda.current_stream(M.device)
    host = []
    for r in rows.tolist():
        dev = steps.instance_masks(torch.tensor([r], dtype=torch.int32, device=M.device), out_size)[0]
        h = torch.empty((V,) + tuple(out_size), dtype=torch.bool, pin_memory=True)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            h.copy_(dev.view(torch.bool), non_blocking=True)
        dev.record_stream(side)
        host.append(h)
        del dev
    side.synchronize()
    return host


class _MinVISDriver(nn.Module):
    """What the VIS and VPS drivers share: settings, dataset checks, normalisation and padding (the image driver's LSJ square padding or
    `size_divisibility`, whichever the config selects), the targets."""

    prefixes: Tuple[str, ...] = ()
    padded_size = InferenceImageGenericSegmentation.padded_size
    image_list = InferenceImageGenericSegmentation.image_list

    def _init_common(self, num_queries, stability_score_thresh, size_divisibility, LSJ_aug_image_size, LSJ_aug_enable_test, pixel_mean,
                     pixel_std, num_frames, num_frames_window_test, test_topk_per_image, merge_on_cpu, dataset_category_info, fused):
        self.num_queries = num_queries
        self.stability_score_thresh = stability_score_thresh
        self.size_divisibility = size_divisibility
        self.LSJ_aug_image_size = LSJ_aug_image_size
        self.LSJ_aug_enable_test = LSJ_aug_enable_test
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(-1, 1, 1), False)
        self.num_frames = num_frames
        self.num_frames_window_test = max(num_frames_window_test, num_frames)
        self.test_topk_per_image = test_topk_per_image
        self.merge_on_cpu = merge_on_cpu          # accepted, no effect: the running sum bounds the memory (module docstring)
        self.dataset_category_info = COMBINED_DATASETS_CATEGORY_INFO if dataset_category_info is None else dataset_category_info
        self.fused = fused
        self.frame_shard = None

    @staticmethod
    def common_config(cfg):
        t = cfg.MODEL.BoxVIS.TEST
        return {
            "num_queries": cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES,
            "stability_score_thresh": cfg.MODEL.MASK_FORMER.TEST.STABILITY_SCORE_THRESH,
            "size_divisibility": cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY,
            "LSJ_aug_image_size": cfg.INPUT.LSJ_AUG.IMAGE_SIZE,
            "LSJ_aug_enable_test": cfg.INPUT.LSJ_AUG.SQUARE_ENABLED,
            "pixel_mean": cfg.MODEL.PIXEL_MEAN,
            "pixel_std": cfg.MODEL.PIXEL_STD,
            "num_frames": cfg.INPUT.SAMPLING_FRAME_NUM,
            "num_frames_window_test": t.NUM_FRAMES_WINDOW,
            "test_topk_per_image": cfg.TEST.DETECTIONS_PER_IMAGE,
            "merge_on_cpu": t.MERGE_ON_CPU,
        }

    @property
    def device(self):
        return self.pixel_mean.device

    def set_frame_shard(self, shard):
        if shard is not None:
            raise NotImplementedError("the MinVIS-style drivers run on one GPU: frame sharding is not built")
        self.frame_shard = None

    def check_dataset(self, dataset_name):
        """Video datasets are named after their class vocabulary ('ytvis21', 'ovis', 'vipseg'; the reference asserts the name is in
        combined_datasets_category_info); a name without one has nothing to score against."""
        if dataset_name not in self.dataset_category_info:
            raise NotImplementedError(f"{type(self).__name__} on {dataset_name!r}: no class vocabulary of that name (video datasets are "
                                      "named after theirs, e.g. 'ytvis21', 'ovis', 'vipseg')")
        if not dataset_name.startswith(self.prefixes):
            raise ValueError(f"Do not support the model inference on {dataset_name}.")
        if self.frame_shard is not None:
            raise NotImplementedError("the MinVIS-style drivers run on one GPU: frame sharding is not built")

    def prepare(self, model, batched_inputs):
        frames = [f.to(self.device).float() for video in batched_inputs for f in video["image"]]
        images = self.image_list(frames)
        targets = model.prepare_targets.process_inference(batched_inputs, tuple(images.tensor.shape[-2:]), self.device,
                                                          getattr(model, "text_prompt_encoder", None), images.image_sizes[0])
        return images, targets

    def clip_loop(self, model, images, targets, vps_matching):
        return run_minvis_loop(model, images, targets, num_frames=self.num_frames, window=self.num_frames_window_test,
                               num_queries=self.num_queries, stability_score_thresh=self.stability_score_thresh,
                               vps_matching=vps_matching, fused=self.fused)

    def steps(self, M, padded, crop):
        return FusedSteps(M, padded, crop) if (self.fused and M.is_cuda) else AtenSteps(M, padded, crop)

    @staticmethod
    def sizes(batched_inputs, images):
        image_size = tuple(int(v) for v in images.image_sizes[0])
        out_size = (int(batched_inputs[0].get("height", image_size[0])), int(batched_inputs[0].get("width", image_size[1])))
        return tuple(int(v) for v in images.tensor.shape[-2:]), image_size, out_size


class InferenceVideoVISFast(_MinVISDriver):
    """VIS with the MinVIS tracker ('ytvis*' / 'ovis*'; TRACKER_TYPE 'minvis').  Returns the reference's dict: image_size, pred_scores,
    pred_labels, pred_masks (a list of bool CPU [V, H0, W0]); records by descending score, ties by flat (row, class) index."""

    prefixes = ("ytvis", "ovis")

    @configurable
    def __init__(self, *, num_queries: int, stability_score_thresh: float, size_divisibility: int, LSJ_aug_image_size: int,
                 LSJ_aug_enable_test: bool, pixel_mean, pixel_std, num_frames: int, num_frames_window_test: int, test_topk_per_image: int,
                 zero_shot_inference: bool = False, tracker_type: str = "minvis", merge_on_cpu: bool = False,
                 dataset_category_info=None, fused: bool = True):
        """`fused=False` runs the ATen formulation of every step on the device (tools/minvis_bench.py's yardstick)."""
        super().__init__()
        self._init_common(num_queries, stability_score_thresh, size_divisibility, LSJ_aug_image_size, LSJ_aug_enable_test, pixel_mean,
                          pixel_std, num_frames, num_frames_window_test, test_topk_per_image, merge_on_cpu, dataset_category_info, fused)
        self.zero_shot_inference = zero_shot_inference
        self.tracker_type = tracker_type

    @classmethod
    def from_config(cls, cfg, dataset_category_info=None):
        d = cls.common_config(cfg)
        d.update(zero_shot_inference=cfg.MODEL.BoxVIS.TEST.ZERO_SHOT_INFERENCE, tracker_type=cfg.MODEL.BoxVIS.TEST.TRACKER_TYPE,
                 dataset_category_info=dataset_category_info)
        return d

    @torch.no_grad()
    def eval(self, model, batched_inputs):
        name = batched_inputs[0]["dataset_name"]
        self.check_dataset(name)
        if self.tracker_type != "minvis":
            raise NotImplementedError(f"TRACKER_TYPE {self.tracker_type!r}: only 'minvis' is built")
        images, targets = self.prepare(model, batched_inputs)
        return self.inference_video_vis_minvis(model, batched_inputs, images, targets)

    def inference_video_vis_minvis(self, model, batched_inputs, images, targets):
        logits, M = self.clip_loop(model, images, targets, vps_matching=False)
        num_classes, start = self.dataset_category_info[batched_inputs[0]["dataset_name"]]
        scores = logits[..., start:start + num_classes].sigmoid()
        return self.postprocess(scores, M, *self.sizes(batched_inputs, images))

    def postprocess(self, mask_scores, M, padded, image_size, out_size):
        """mask_scores [Q', C] (after the sigmoid), M [Q', V, h, w] mean mask logits -> the reference's dict (:299-351)."""
        V = int(M.shape[1])
        rows = mask_scores.max(-1)[0].sort(descending=True)[1][:self.test_topk_per_image]
        mask_scores = mask_scores[rows]
        if self.zero_shot_inference:
            mask_scores = (mask_scores * 20).softmax(-1)
        C = mask_scores.shape[-1]
        num_topk = min(self.test_topk_per_image, max(int((mask_scores > 2 * (1.0 / C)).sum()), 5), mask_scores.numel())
        flat = mask_scores.flatten()
        order = torch.sort(flat, descending=True, stable=True)[1][:num_topk]     # topk: descending score, ties by flat index
        scores, labels = flat[order], order % C
        rec_rows = rows[torch.div(order, C, rounding_mode="floor")]
        uniq, inv = torch.unique(rec_rows, return_inverse=True)                 # a repeated row is computed once
        steps = self.steps(M, padded, image_size)
        st = steps.mask_stats(uniq, max(int(V / 10.0), 1))
        quality = (st[:, 0].float() / st[:, 1].clamp(min=1).float()).clamp(min=0.1)
        scores = scores * quality[inv]
        final = torch.sort(scores, descending=True, stable=True)[1]            # by the final score, ties by flat index
        scores, labels, inv = scores[final], labels[final], inv[final]
        masks = _masks_to_host(steps, uniq, out_size)
        return {"image_size": out_size, "pred_scores": scores.tolist(), "pred_labels": labels.tolist(),
                "pred_masks": [masks[j] for j in inv.tolist()]}


class InferenceVideoVPS(_MinVISDriver):
    """Online VPS ('vipseg*').  Returns the reference's dict: image_size, pred_masks [V, H0, W0] int32 segment ids (CPU), segments_infos,
    pred_ids, task 'vps'; the output size is the 720p form of the input's (change_to_720p)."""

    prefixes = ("vipseg",)

    @configurable
    def __init__(self, *, num_queries: int, stability_score_thresh: float, size_divisibility: int, LSJ_aug_image_size: int,
                 LSJ_aug_enable_test: bool, pixel_mean, pixel_std, num_frames: int, num_frames_window_test: int, test_topk_per_image: int,
                 object_mask_threshold: float, overlap_threshold: float, thing_dataset_ids=(), change_to_720p: bool = True,
                 merge_on_cpu: bool = False, dataset_category_info=None, fused: bool = True):
        """`thing_dataset_ids`: the category ids (1-based, the keys of the reference's metadata.thing_dataset_id_to_contiguous_id) that
        are things; the driver refuses to run without them (every thing would be merged as stuff)."""
        super().__init__()
        self._init_common(num_queries, stability_score_thresh, size_divisibility, LSJ_aug_image_size, LSJ_aug_enable_test, pixel_mean,
                          pixel_std, num_frames, num_frames_window_test, test_topk_per_image, merge_on_cpu, dataset_category_info, fused)
        self.object_mask_threshold = object_mask_threshold
        self.overlap_threshold = overlap_threshold
        self.thing_dataset_ids = [int(c) for c in thing_dataset_ids]
        self.change_to_720p = change_to_720p

    @classmethod
    def from_config(cls, cfg, thing_dataset_ids=(), dataset_category_info=None):
        d = cls.common_config(cfg)
        d.update(object_mask_threshold=cfg.MODEL.MASK_FORMER.TEST.OBJECT_MASK_THRESHOLD,
                 overlap_threshold=cfg.MODEL.MASK_FORMER.TEST.OVERLAP_THRESHOLD, thing_dataset_ids=thing_dataset_ids,
                 dataset_category_info=dataset_category_info)
        return d

    def check_things(self):
        if not self.thing_dataset_ids:
            raise ValueError("panoptic video inference needs the thing categories: set thing_dataset_ids (the reference reads them from "
                             "metadata.thing_dataset_id_to_contiguous_id)")

    @torch.no_grad()
    def eval(self, model, batched_inputs):
        self.check_dataset(batched_inputs[0]["dataset_name"])
        self.check_things()
        images, targets = self.prepare(model, batched_inputs)
        return self.inference_video_vps_online(model, batched_inputs, images, targets)

    def inference_video_vps_online(self, model, batched_inputs, images, targets):
        logits, M = self.clip_loop(model, images, targets, vps_matching=True)
        num_classes, start = self.dataset_category_info[batched_inputs[0]["dataset_name"]]
        pred_cls = logits[..., start:start + num_classes].sigmoid()
        padded, image_size, out_size = self.sizes(batched_inputs, images)
        if self.change_to_720p:
            out_size = (720, int(720 * out_size[1] / out_size[0]))
        return self.postprocess(pred_cls, M, padded, image_size, out_size)

    def postprocess(self, pred_cls, M, padded, image_size, out_size):
        """pred_cls [Q', C] (after the sigmoid), M [Q', V, h, w] mean mask logits -> the reference's dict (:309-406)."""
        self.check_things()
        V = int(M.shape[1])
        scores, labels = pred_cls.max(-1)
        k = self.test_topk_per_image
        if scores.numel() < k:
            raise ValueError(f"the keep rule takes the {k}-th best score (TEST.DETECTIONS_PER_IMAGE = {k}) but the video has "
                             f"{scores.numel()} rows; lower TEST.DETECTIONS_PER_IMAGE (MODEL.MASK_FORMER.TEST.OBJECT_MASK_THRESHOLD = "
                             f"{self.object_mask_threshold} is the other bound of the rule)")
        keep = scores > max(self.object_mask_threshold, scores.topk(k=k)[0][-1])
        rows = torch.nonzero(keep).flatten()
        cur_scores, cur_classes = scores[keep], labels[keep]
        result = {"image_size": out_size, "segments_infos": [], "pred_ids": [], "task": "vps"}
        if rows.numel() == 0:
            result["pred_masks"] = torch.zeros((V,) + tuple(out_size), dtype=torch.int32)
            return result
        steps = self.steps(M, padded, image_size)
        st = steps.mask_stats(rows, VPS_QUALITY_STEP)
        cur_scores = cur_scores + 0.5 * (st[:, 0].float() / st[:, 1].clamp(min=1).float())
        ids = steps.panoptic_ids(rows, cur_scores)
        counts = steps.panoptic_counts(rows, ids, out_size)
        host = torch.cat([counts.long().flatten().cpu(), cur_classes.long().cpu() + 1, rows.long().cpu()]).numpy()
        K = int(rows.numel())
        classes, ids_host = host[3 * K:4 * K], host[4 * K:]
        lut, infos = panoptic_segments(host[:3 * K].reshape(K, 3), classes, set(self.thing_dataset_ids), self.overlap_threshold)
        first = {}
        for j, v in enumerate(lut):
            first.setdefault(v, j)
        result["segments_infos"] = infos
        result["pred_ids"] = [int(ids_host[first[info["id"]]]) for info in infos]
        result["pred_masks"] = steps.panoptic_paint(rows, ids, lut, out_size).cpu()
        return result


def instances_to_coco_json_video(inputs, outputs):
    """The YTVIS evaluator's conversion of one video's VIS dict (univs/evaluation/ytvis_evaluation.py:294-333): one record per
    (score, label, masks) with a COCO RLE per frame (counts as str), on the device RLE (results.rle_encode_masks)."""
    assert len(inputs) == 1, "More than one inputs are loaded for inference!"
    video_id = int(inputs[0]["video_id"])
    height, width = int(inputs[0]["height"]), int(inputs[0]["width"])
    out, cache = [], {}
    for s, l, m in zip(outputs["pred_scores"], outputs["pred_labels"], outputs["pred_masks"]):
        if id(m) not in cache:                    # (records of one row share its masks)
            cache[id(m)] = (m, rle_encode_masks(m))
        segms = [dict(r) for r in cache[id(m)][1]]
        out.append({"video_id": video_id, "score": s, "category_id": l, "segmentations": segms, "height": height, "width": width})
    return out
