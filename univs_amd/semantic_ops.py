"""Wrapper of the fifth header (include/univs_semantic_hip.h): the mask-quality counts of the semantic-feature decoder
(inference/semantic_to_mask.py), and the same counts from torch ops.

  semantic_quality_counts        the HIP kernel (csrc/semantic_decode.hip) behind `ops._call`: GPU tensors only (a CPU tensor raises), None
                                 where the kernel does not cover the call
  semantic_quality_counts_aten   the same tensor from torch ops on any device: the CPU path, the fall-back, the yardstick

mask_embed is float32 [T, N, C], features float32 [T, C, h, w] (or [T, C, HW]).  Both return int32 [N, 2]: over the frames
0, t_step, 2 t_step, ... < T and all their pixels, the number of logits sum_c mask_embed[t, n, c] * features[t, c, p] of row n that are
> t_hi, and > t_lo (strict): numerator and denominator of the reference's `calculate_mask_quality_scores` on
`mask_logits[:, ::temporal_stride]` (semantic_feature_to_mask.py:9-12, :109).  The kernel stores no logit; its logits are those of
`ops.mask_decode` under `mask_decode_impl=1` bit for bit, so its counts are that tensor's counts exactly.
"""
import torch

from . import _lib, ops


def _check(name, mask_embed, features, t_step):
    if mask_embed.dtype != torch.float32 or features.dtype != torch.float32:
        raise RuntimeError(f"{name}: float32 only")
    if mask_embed.dim() != 3 or features.dim() not in (3, 4) or tuple(features.shape[:2]) != (mask_embed.shape[0], mask_embed.shape[2]):
        raise RuntimeError(f"{name}: shape mismatch {tuple(mask_embed.shape)} vs {tuple(features.shape)}: [T, N, C] and [T, C, h, w]")
    if 0 in mask_embed.shape or 0 in features.shape:
        raise RuntimeError(f"{name}: empty tensors {tuple(mask_embed.shape)}, {tuple(features.shape)}")
    if int(t_step) != t_step or int(t_step) < 1:
        raise RuntimeError(f"{name}: t_step {t_step}")


def semantic_quality_counts(mask_embed, features, t_step, t_hi=1.0, t_lo=-1.0):
    """counts int32 [N, 2] from csrc/semantic_decode.hip on the tensors' device and current stream; None where the kernel does not cover
    the sizes (include/univs_semantic_hip.h states them): the caller keeps `semantic_quality_counts_aten`.  CPU tensors raise, as in
    every wrapper of ops.py."""
    name = "semantic_quality_counts"
    ops._inference_only(name, mask_embed, features)
    ops._require_gpu(name, mask_embed, features)
    _check(name, mask_embed, features, t_step)
    if features.device != mask_embed.device:
        raise RuntimeError(f"{name}: mask_embed on {mask_embed.device}, features on {features.device}")
    T, N, C = (int(v) for v in mask_embed.shape)
    HW = features.numel() // (T * C)
    if HW >= 2 ** 31:                                                # (beyond the entry's int)
        return None
    counts = torch.empty((N, 2), dtype=torch.int32, device=mask_embed.device)      # (zeroed by the entry, on this stream)
    ok = ops._call(name, _lib.load().univs_semantic_quality_counts_f32, mask_embed, ops._ptr(mask_embed), ops._ptr(features), T, N, C, HW,
                   int(t_step), float(t_hi), float(t_lo), ops._ptr(counts))
    return counts if ok else None


def semantic_quality_counts_aten(mask_embed, features, t_step, t_hi=1.0, t_lo=-1.0):
    """counts int32 [N, 2] on the tensors' device, CPU or GPU, one walked frame at a time: the peak is one frame's logits [N, HW] and
    its two boolean maps, not the stack."""
    _check("semantic_quality_counts_aten", mask_embed, features, t_step)
    T, N, _ = mask_embed.shape
    counts = torch.zeros((N, 2), dtype=torch.int64, device=mask_embed.device)
    for t in range(0, int(T), int(t_step)):
        logits = torch.einsum("nc,cp->np", mask_embed[t], features[t].flatten(1))
        counts[:, 0] += (logits > t_hi).sum(-1)
        counts[:, 1] += (logits > t_lo).sum(-1)
    return counts.to(torch.int32)
