"""The consumer of the semantic-extraction files: object tokens and compressed mask features back into class logits and mask logits.

Counterpart of the reference's `ConvertSemanticFeatureToMask` (semantic_feature_to_mask.py:30-116; its `plot_masks` and `__main__` are
a plotting demo and are not restated).  video_semantic_extraction.py writes, per video, `<video>._obj_tokens_<r>_<t>.pt` [V', C, N] and
`<video>._compression_mask_features_<r>_<t>.pt` [V', C, hc, wc]; `convert` applies the predictor's own heads to them:

    tokens -> decoder_norm -> mask_embed MLP                      the mask embeddings [T, N, C]
           -> vis2text_projection, cosine against the CLIP table, * exp(cls_temp)     class logits [N, T, K]
    confidence  sigmoid(class logits)[..., 1000:] maximised over frames and classes > apply_cls_thres
    quality     |{logit > 1}| / max(|{logit > -1}|, 1) over every temporal_stride-th frame > apply_mask_quality_thres
    kept rows   both; their mask logits [n, T, hc, wc]

What is organised differently (same values, shapes and dtypes).  The reference builds the whole logit stack [N, T, hc, wc] (3.5 GB at
T = 300, N = 200, 90 x 160), then two boolean stacks of its strided view, to decide which rows to keep.  Here the two counts per row
come from semantic_ops.semantic_quality_counts (csrc/semantic_decode.hip: the contraction with a counting epilogue, no logit stored),
and only the kept rows are decoded afterwards, by ops.mask_decode under the exact-f32 setting -- the same kernel templates, one fmaf
chain per logit, so the logits returned are the very values that were counted.  decoder_norm + the MLP run as the one launch of the
decoder's prediction head (layers.MLP: `in_norm=`, `want_normed=True`); the class side stays on the existing Linear and ATen operators
(about a twelfth of the mask side's arithmetic at ratio 8).

Deliberate differences from the reference:
  * inputs are moved to the module's device (the files hold CPU tensors; the reference leaves that to its caller);
  * `indices` lives on the module's device in both branches (the reference's `arange` of the all-rows branch is a CPU tensor);
  * K <= 1000 classes with `only_high_conf_masks` raises a ValueError naming K (the reference fails inside `max` of an empty slice);
  * `load_pretrained_checkpoint` returns the matched and skipped names and logs them once instead of printing a line per parameter;
  * `clip_class_embed_path` may be a tensor and `pretrained_ckpt` a state dict (or None: the initial values stay);
  * on CPU tensors the whole path runs in ATen.

    python -m univs_amd.inference.semantic_to_mask --obj_tokens V._obj_tokens_8_1.pt --mask_features V._compression_mask_features_8_1.pt \\
        --ckpt model.pth --clip_emb cls_emb.pth --out result.pt [--all]
"""
import argparse
import logging
import os

import torch
import torch.nn.functional as F
from torch import nn

from .. import ops, semantic_ops
from ..layers import MLP, linear

logger = logging.getLogger(__name__)

PREDICTOR_PREFIX = "sem_seg_head.predictor."
FIRST_ENTITY_CLASS = 1000       # the CLIP table starts with the 1000 ImageNet names, which the confidence ignores (:107)


class ConvertSemanticFeatureToMask(nn.Module):
    """The reference's keywords, defaults, submodule names and state-dict layout (semantic_feature_to_mask.py:31-59)."""

    def __init__(self, hidden_dim=256, mask_dim=256, text_emb_dim=640, apply_cls_thres=0.65, apply_mask_quality_thres=0.85,
                 temporal_stride=10, clip_class_embed_path="datasets/concept_emb/combined_datasets_cls_emb_rn50x4.pth",
                 pretrained_ckpt="pretrained/univs_v2_cvpr/univs_swinb_stage3_f7_wosquare_ema.pth", device="cuda"):
        super().__init__()
        self.device = torch.device(device if torch.cuda.is_available() else "cpu")
        self.decoder_norm = nn.LayerNorm(hidden_dim)
        self.mask_embed = MLP(hidden_dim, hidden_dim, mask_dim, 3)
        self.vis2text_projection = nn.Linear(hidden_dim, text_emb_dim)
        self.cls_temp = nn.Embedding(1, 1)
        self.to(self.device)
        # text embeddings of the category names from the CLIP text encoder [K, text_emb_dim]: a tensor, or the path of a torch-saved one
        if not isinstance(clip_class_embed_path, torch.Tensor):
            clip_class_embed_path = torch.load(clip_class_embed_path, map_location="cpu")
        self.clip_cls_text_emb = clip_class_embed_path.to(self.device)
        self._clip_norm_cache = None
        self.apply_cls_thres = apply_cls_thres
        self.apply_mask_quality_thres = apply_mask_quality_thres
        self.temporal_stride = temporal_stride
        self.matched, self.skipped = [], []
        if pretrained_ckpt is not None:
            self.load_pretrained_checkpoint(pretrained_ckpt)

    @classmethod
    def from_predictor(cls, predictor, **thresholds):
        """A converter that SHARES the parameters of a built `VideoMultiScaleMaskedTransformerDecoderUniVS` (its decoder_norm, mask_embed,
        vis2text_projection, cls_temp and CLIP table); `thresholds`: apply_cls_thres, apply_mask_quality_thres, temporal_stride."""
        unknown = set(thresholds) - {"apply_cls_thres", "apply_mask_quality_thres", "temporal_stride"}
        if unknown:
            raise TypeError(f"from_predictor: unknown keywords {sorted(unknown)}")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.decoder_norm, self.mask_embed = predictor.decoder_norm, predictor.mask_embed
        self.vis2text_projection, self.cls_temp = predictor.vis2text_projection, predictor.cls_temp
        self.device = self.decoder_norm.weight.device
        self.clip_cls_text_emb = predictor.clip_cls_text_emb.to(self.device)
        self._clip_norm_cache = None
        self.apply_cls_thres = thresholds.get("apply_cls_thres", 0.65)
        self.apply_mask_quality_thres = thresholds.get("apply_mask_quality_thres", 0.85)
        self.temporal_stride = thresholds.get("temporal_stride", 10)
        self.matched, self.skipped = [], []
        return self

    def load_pretrained_checkpoint(self, pretrained_ckpt):
        """The reference's rule (:61-88) on a path or a loaded dict: `["model"]` if present; a parameter takes the FIRST checkpoint key
        with name == key.replace("sem_seg_head.predictor.", "") and an equal size; everything else keeps its initial value.  Returns
        (matched names, skipped names), logged once."""
        pretrained = torch.load(pretrained_ckpt, map_location="cpu") if isinstance(pretrained_ckpt, (str, os.PathLike)) else pretrained_ckpt
        if not isinstance(pretrained, dict):
            raise ValueError(f"load_pretrained_checkpoint: a dict of tensors or {{'model': ...}} is needed, got {type(pretrained).__name__}")
        weights = pretrained["model"] if "model" in pretrained else pretrained
        keys = list(weights.keys())
        matched, skipped = [], []
        with torch.no_grad():
            for name, param in self.state_dict().items():
                source = next((k for k in keys if name == k.replace(PREDICTOR_PREFIX, "") and hasattr(weights[k], "size")
                               and param.size() == weights[k].size()), None)
                if source is None:
                    skipped.append(name)
                else:
                    param.copy_(torch.as_tensor(weights[source]))
                    matched.append(name)
        self._clip_norm_cache = None
        self.matched, self.skipped = matched, skipped
        logger.info("semantic_to_mask: %d parameters from the checkpoint %s; %d keep their initial values (absent or size mismatch) %s",
                    len(matched), matched, len(skipped), skipped)
        return matched, skipped

    def _clip_normalized(self, like):
        c = self._clip_norm_cache
        if c is None or c.device != like.device or c.dtype != like.dtype:
            c = F.normalize(self.clip_cls_text_emb.to(like), p=2, dim=-1).detach()
            self._clip_norm_cache = c
        return c

    @torch.no_grad()
    def heads(self, obj_tokens):
        """obj_tokens [T, C, N] on the module's device -> (class logits [N, T, K], mask embeddings [T, N, C] contiguous) (:92-101)."""
        x = obj_tokens.transpose(1, 2)                                                # [T, N, C]
        mask_embed, normed = self.mask_embed(x, in_norm=self.decoder_norm, want_normed=True)
        cls_logits = linear(normed, self.vis2text_projection.weight, self.vis2text_projection.bias)
        clip = self._clip_normalized(cls_logits)
        cls_logits = F.normalize(cls_logits, p=2, dim=-1)
        cls_logits = torch.einsum("tnc,kc->tnk", cls_logits, clip)
        cls_logits = cls_logits * self.cls_temp.weight.exp()
        return cls_logits.transpose(0, 1), mask_embed.contiguous()

    @torch.no_grad()
    def quality_counts(self, mask_embed, mask_feats):
        """int32 [N, 2]: the fused kernel on the GPU where it covers the sizes, else the ATen formulation."""
        counts = None
        if mask_embed.is_cuda:
            counts = semantic_ops.semantic_quality_counts(mask_embed, mask_feats, self.temporal_stride)
        if counts is None:
            counts = semantic_ops.semantic_quality_counts_aten(mask_embed, mask_feats, self.temporal_stride)
        return counts

    @torch.no_grad()
    def scores(self, cls_logits, mask_embed, mask_feats):
        """(confidence float32 [N], quality float32 [N], counts int32 [N, 2]) of every row (:106-109)."""
        K = int(cls_logits.shape[-1])
        if K <= FIRST_ENTITY_CLASS:
            raise ValueError(f"the confidence reads the classes from {FIRST_ENTITY_CLASS} on, but the CLIP table has K = {K} rows")
        confidence = cls_logits.sigmoid()[..., FIRST_ENTITY_CLASS:].flatten(1).max(1)[0]
        counts = self.quality_counts(mask_embed, mask_feats)
        c = counts.to(torch.int64)
        quality = c[:, 0] / c[:, 1].clamp(min=1)                                      # (int64 / int64: the reference's float32 quotient)
        return confidence, quality, counts

    @staticmethod
    def decode(mask_embed, mask_feats):
        """mask logits [n, T, h, w] of the rows of mask_embed [T, n, C]: on the GPU ops.mask_decode under the exact-f32 setting (restored
        afterwards) -- the arithmetic the counts were taken from."""
        if not mask_embed.is_cuda:
            return torch.einsum("tnc,tchw->tnhw", mask_embed, mask_feats).transpose(0, 1)
        with ops.configured(mask_decode_impl=1):
            return ops.mask_decode(mask_embed, mask_feats)

    @torch.no_grad()
    def convert(self, mask_feats, obj_tokens, only_high_conf_masks=True):
        """mask_feats [T, C, hc, wc], obj_tokens [T, C, N] -> (cls_logits [n, T, K], mask_logits [n, T, hc, wc], indices int64 [n]) of the
        rows that pass both filters, or of all rows with `only_high_conf_masks=False` (:90-116)."""
        mask_feats = mask_feats.to(self.device).contiguous()
        obj_tokens = obj_tokens.to(self.device)
        cls_logits, mask_embed = self.heads(obj_tokens)
        if not only_high_conf_masks:
            return cls_logits, self.decode(mask_embed, mask_feats), torch.arange(mask_embed.shape[1], device=self.device)
        confidence, quality, _ = self.scores(cls_logits, mask_embed, mask_feats)
        keep = (confidence > self.apply_cls_thres) & (quality > self.apply_mask_quality_thres)
        indices = torch.nonzero(keep).reshape(-1)
        return cls_logits[indices], self.decode(mask_embed[:, indices].contiguous(), mask_feats), indices


def decode_files(obj_tokens, mask_features, ckpt, clip_emb, out=None, all_rows=False, device="cuda", **keywords):
    """The two files of one video -> {"cls_logits", "mask_logits", "indices"} as contiguous CPU tensors, saved to `out` when given.
    `keywords`: hidden_dim, mask_dim, text_emb_dim, the two thresholds and temporal_stride of `ConvertSemanticFeatureToMask`."""
    converter = ConvertSemanticFeatureToMask(clip_class_embed_path=clip_emb, pretrained_ckpt=ckpt, device=device, **keywords)
    tokens = torch.load(obj_tokens, map_location="cpu")
    feats = torch.load(mask_features, map_location="cpu")
    cls_logits, mask_logits, indices = converter.convert(feats, tokens, only_high_conf_masks=not all_rows)
    result = {"cls_logits": cls_logits.contiguous().cpu(), "mask_logits": mask_logits.contiguous().cpu(), "indices": indices.contiguous().cpu()}
    if out is not None:
        torch.save(result, out)
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(description="Decode the two semantic-extraction files of a video into class logits and mask logits.")
    ap.add_argument("--obj_tokens", required=True)
    ap.add_argument("--mask_features", required=True)
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--clip_emb", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--all", action="store_true", help="every row, not only the confident high-quality ones")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--hidden_dim", type=int, default=256)
    ap.add_argument("--mask_dim", type=int, default=256)
    ap.add_argument("--text_emb_dim", type=int, default=640)
    ap.add_argument("--cls_thres", type=float, default=0.65)
    ap.add_argument("--mask_quality_thres", type=float, default=0.85)
    ap.add_argument("--temporal_stride", type=int, default=10)
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    r = decode_files(a.obj_tokens, a.mask_features, a.ckpt, a.clip_emb, out=a.out, all_rows=a.all, device=a.device, hidden_dim=a.hidden_dim,
                     mask_dim=a.mask_dim, text_emb_dim=a.text_emb_dim, apply_cls_thres=a.cls_thres,
                     apply_mask_quality_thres=a.mask_quality_thres, temporal_stride=a.temporal_stride)
    logger.info("semantic_to_mask: kept %d rows -> %s", int(r["indices"].numel()), a.out)


if __name__ == "__main__":
    main()
