"""Semantic extraction (MODEL.UniVS.TEST.SEMANTIC_EXTRACTION.ENABLE): UniVS as a feature extractor that exports, per video, the learnable
object tokens and a spatially compressed copy of the mask features -- the two files the reference's `semantic_feature_to_mask.py` later
decodes into masks and classes.

Counterpart of the reference's driver:

    InferenceVideoSemanticExtraction   univs/inference/inference_video_semantic_extraction.py
        eval                :148-179   normalise, pad, targets
        inference_video     :181-262   the clip loop (extract), the resampling of the mask features (the steps below), the two files (save)

The clip loop.  Clips run at stride `num_frames`; the backbone runs once per window of 2 * num_frames frames; the head is called with
targets[0]["first_frame_idx"] / ["frame_indices"] of the clip, the last clip may be shorter.  The head (univs_decoder.py under
`semantic_extraction_enable`) returns `pred_embds` [T, C, N] and `mask_features` [T, C, h, w].

The resampling.  The reference up-samples each clip's mask features to the padded input size ([T, 256, Hp, Wp] fp32: 4.8 GB for five
736 x 1280 frames), crops, keeps one pixel in ratio^2 with a nearest resize, concatenates the clips and keeps every t_itv-th frame.  Here
the per-video tensor [ceil(V / t_itv), C, hc, wc] is allocated once and each clip's kept frames are written straight into their rows:
on the GPU by one gather (`FusedSteps`: ops.bilinear_crop_nearest, csrc/semantic_extract.hip -- the up-sampled stack is never built and
the frames the temporal ratio drops are not computed), on the CPU and where the kernel does not cover the shape by the reference's three
expressions (`AtenSteps`).

One deliberate difference: the saved tensors are CPU tensors (the reference pickles device tensors, which a machine without that device
cannot load), contiguous (the reference pickles the `[::t_itv]` view and with it the whole storage); values, shapes, dtypes and file names
are the reference's.  The driver runs on one GPU: it raises if a frame shard is set.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from ..registry import configurable
from .image_generic_seg import InferenceImageGenericSegmentation, fused_or_aten


class AtenSteps:
    """The reference's formulation (:220-235): F.interpolate(bilinear) to the padded size, crop, F.interpolate(nearest).  The CPU path of
    the driver, the fall-back for shapes the kernel does not cover, and the yardstick of the tests and of tools/semantic_bench.py."""

    def __init__(self, padded, crop, size):
        self.padded, self.crop, self.size = (tuple(int(v) for v in s) for s in (padded, crop, size))

    def compress(self, mask_features, t_first, t_step, out):
        """out [K, C, hc, wc] <- the compressed features of frames t_first, t_first + t_step, ... of the clip."""
        U = F.interpolate(mask_features, size=self.padded, mode="bilinear", align_corners=False)
        U = U[..., :self.crop[0], :self.crop[1]]
        out.copy_(F.interpolate(U, size=self.size, mode="nearest")[t_first::t_step])
        return out


class FusedSteps(AtenSteps):
    """The same step as one gather (ops.bilinear_crop_nearest); `AtenSteps` only where the kernel does not cover the shape (None)."""

    def compress(self, mask_features, t_first, t_step, out):
        r = ops.bilinear_crop_nearest(mask_features, self.padded, self.crop, self.size, t_first=t_first, t_step=t_step, out=out)
        return fused_or_aten(r, super().compress, mask_features, t_first, t_step, out)


class InferenceVideoSemanticExtraction(nn.Module):
    """Extracts the learnable object tokens [V', C, N] and the compressed mask features [V', C, hc, wc] of one video (V' = ceil(V / t_itv),
    hc = int(height / ratio), wc = int(width / ratio)) and saves them as `<video_id>._obj_tokens_<ratio>_<t_itv>.pt` and
    `<video_id>._compression_mask_features_<ratio>_<t_itv>.pt`."""

    padded_size = InferenceImageGenericSegmentation.padded_size
    image_list = InferenceImageGenericSegmentation.image_list

    @configurable
    def __init__(self, *, hidden_dim: int, num_queries: int, overlap_threshold: float, overlap_threshold_entity: float,
                 stability_score_thresh: float, size_divisibility: int, LSJ_aug_image_size: int, LSJ_aug_enable_test: bool,
                 sem_seg_postprocess_before_inference: bool, pixel_mean, pixel_std, num_frames: int, num_classes: int, metadata=None,
                 semantic_extraction_enable: bool = True, semantic_extraction_compression_ratio: int = 8,
                 semantic_extraction_compression_ratio_temporal: int = 1, semantic_extraction_output_dir: str = "", fused: bool = True):
        """The reference's keywords (:58-81; `metadata` is kept and unused, as there).  `fused=False` runs the ATen formulation on the
        device (tools/semantic_bench.py's yardstick)."""
        super().__init__()
        self.hidden_dim = hidden_dim
        self.num_queries = num_queries
        self.overlap_threshold = overlap_threshold
        self.overlap_threshold_entity = overlap_threshold_entity
        self.stability_score_thresh = stability_score_thresh
        self.metadata = metadata
        self.size_divisibility = size_divisibility
        self.LSJ_aug_image_size = LSJ_aug_image_size
        self.LSJ_aug_enable_test = LSJ_aug_enable_test
        self.sem_seg_postprocess_before_inference = sem_seg_postprocess_before_inference
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(-1, 1, 1), False)
        self.num_frames = num_frames
        self.num_classes = num_classes
        self.num_frames_window_test = 2 * num_frames
        self.semantic_extraction_enable = semantic_extraction_enable
        self.semantic_extraction_compression_ratio = semantic_extraction_compression_ratio
        self.semantic_extraction_compression_ratio_temporal = semantic_extraction_compression_ratio_temporal
        self.semantic_extraction_output_dir = semantic_extraction_output_dir
        self.fused = fused
        self.frame_shard = None

    @classmethod
    def from_config(cls, cfg, metadata=None):
        se = cfg.MODEL.UniVS.TEST.SEMANTIC_EXTRACTION
        return {
            "hidden_dim": cfg.MODEL.MASK_FORMER.HIDDEN_DIM,
            "num_queries": cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES,
            "overlap_threshold": cfg.MODEL.MASK_FORMER.TEST.OVERLAP_THRESHOLD,
            "overlap_threshold_entity": cfg.MODEL.MASK_FORMER.TEST.OVERLAP_THRESHOLD_ENTITY,
            "stability_score_thresh": cfg.MODEL.MASK_FORMER.TEST.STABILITY_SCORE_THRESH,
            "metadata": metadata,
            "size_divisibility": cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY,
            "LSJ_aug_image_size": cfg.INPUT.LSJ_AUG.IMAGE_SIZE,
            "LSJ_aug_enable_test": cfg.INPUT.LSJ_AUG.SQUARE_ENABLED,
            "sem_seg_postprocess_before_inference": cfg.MODEL.MASK_FORMER.TEST.SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE,
            "pixel_mean": cfg.MODEL.PIXEL_MEAN,
            "pixel_std": cfg.MODEL.PIXEL_STD,
            "num_frames": cfg.INPUT.SAMPLING_FRAME_NUM,
            "num_classes": cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES,
            "semantic_extraction_enable": se.ENABLE,
            "semantic_extraction_compression_ratio": se.COMPRESSION_RATIO,
            "semantic_extraction_compression_ratio_temporal": se.COMPRESSION_RATIO_TEMPORAL,
            "semantic_extraction_output_dir": se.OUTPUT_DIR,
        }

    @property
    def device(self):
        return self.pixel_mean.device

    def set_frame_shard(self, shard):
        if shard is not None:
            raise NotImplementedError("semantic extraction runs on one GPU: frame sharding is not built")
        self.frame_shard = None

    @torch.no_grad()
    def eval(self, model, batched_inputs):
        """batched_inputs: the mapper's one video {"image": [CHW tensors 0..255], "video_len", "video_id", "file_names", optional
        "height" / "width", ...}.  Writes the two files and returns None, as the reference does."""
        if self.frame_shard is not None:
            raise NotImplementedError("semantic extraction runs on one GPU: frame sharding is not built")
        frames = [f.to(self.device).float() for video in batched_inputs for f in video["image"]]
        images = self.image_list(frames)
        targets = model.prepare_targets.process_inference(batched_inputs, tuple(images.tensor.shape[-2:]), self.device,
                                                          getattr(model, "text_prompt_encoder", None), images.image_sizes[0])
        return self.inference_video(model, batched_inputs, images, targets)

    def inference_video(self, model, batched_inputs, images, targets):
        assert "video_id" in batched_inputs[0]
        obj_tokens, features = self.extract(model, batched_inputs, images, targets)
        self.save(batched_inputs[0]["video_id"], targets[0]["file_names"], obj_tokens, features)

    def steps(self, mask_features, padded, crop, size):
        use_kernel = self.fused and mask_features.is_cuda and mask_features.dtype == torch.float32
        return (FusedSteps if use_kernel else AtenSteps)(padded, crop, size)

    def compressed_size(self, batched_inputs, images):
        """(hc, wc) = (int(height / ratio), int(width / ratio)) of the record's output size, which defaults to the un-padded image size."""
        image_size = images.image_sizes[0]
        out_height = batched_inputs[0].get("height", image_size[0])
        out_width = batched_inputs[0].get("width", image_size[1])
        s_itv = self.semantic_extraction_compression_ratio
        return int(out_height / s_itv), int(out_width / s_itv)

    def extract(self, model, batched_inputs, images, targets):
        """The clip loop (:194-246) -> (obj_tokens [V', C, N], features [V', C, hc, wc]) on the model's device, V' = ceil(V / t_itv)."""
        x = images.tensor
        V, T = int(x.shape[0]), int(self.num_frames)
        video_len = int(batched_inputs[0]["video_len"])
        padded = tuple(int(v) for v in x.shape[-2:])
        crop = tuple(int(v) for v in images.image_sizes[0])
        size = self.compressed_size(batched_inputs, images)
        t_itv = int(self.semantic_extraction_compression_ratio_temporal)
        tokens, features, steps = [], None, None
        start, end, feats_w = 0, 0, None
        seen = 0
        for i in range(0, V, T):
            targets[0]["first_frame_idx"] = i
            targets[0]["frame_indices"] = torch.arange(i, min(i + T, V))
            if i + T > end:
                start, end = i, i + self.num_frames_window_test
                feats_w = model.backbone(x[start:end])
            clip = {k: v[i - start:i - start + T] for k, v in feats_w.items()}
            out = model.sem_seg_head(clip, targets=targets)
            obj_tokens, mask_features = out["pred_embds"], out["mask_features"]       # [T', C, N], [T', C, h, w]
            n = int(mask_features.shape[0])
            if features is None:
                features = torch.empty((len(range(0, V, t_itv)), int(mask_features.shape[1])) + size, dtype=mask_features.dtype,
                                       device=mask_features.device)
                steps = self.steps(mask_features, padded, crop, size)
            t_first = (-i) % t_itv                      # the clip's first frame that [::t_itv] over the video keeps
            rows = len(range(t_first, n, t_itv))
            if rows:
                r0 = (i + t_first) // t_itv
                steps.compress(mask_features, t_first, t_itv, features[r0:r0 + rows])
            tokens.append(obj_tokens)
            seen += int(obj_tokens.shape[0])
            del out, mask_features
        assert video_len == seen, (video_len, seen)
        return torch.cat(tokens)[::t_itv], features

    def output_dir(self, file_names):
        """OUTPUT_DIR, else the grand-parent path of the first frame's file name with 'raw' -> 'semantic_extraction' (:249-255)."""
        if self.semantic_extraction_output_dir is None or len(self.semantic_extraction_output_dir) == 0:
            return "/".join(file_names[0].split("/")[:-2]).replace("raw", "semantic_extraction")
        return self.semantic_extraction_output_dir

    def file_names(self, video_id):
        s_itv, t_itv = self.semantic_extraction_compression_ratio, self.semantic_extraction_compression_ratio_temporal
        return video_id + f"._obj_tokens_{s_itv}_{t_itv}.pt", video_id + f"._compression_mask_features_{s_itv}_{t_itv}.pt"

    def save(self, video_id, file_names, obj_tokens, features):
        """The two `.pt` files (:256-262) as contiguous CPU tensors; one copy to the host per tensor and video.  Returns their paths."""
        out_dir = self.output_dir(file_names)
        os.makedirs(out_dir, exist_ok=True)
        paths = tuple(os.path.join(out_dir, n) for n in self.file_names(video_id))
        for path, t in zip(paths, (obj_tokens, features)):
            torch.save(t.detach().contiguous().cpu(), path)
        return paths
