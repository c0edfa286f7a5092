"""Wrapper of the sixth header (include/univs_encoder_hip.h): the two projections at the head of a deformable-encoder layer in one launch.

  linear_pair_blocked    value_proj on `src` and the merged sampling-offset / attention-weight projection on `src + pos`, pos one frame's
                         table, from ONE read of src (csrc/linear_pair_f16x3.hip): `src + pos` is never a tensor.  Each output has the bits
                         of `ops.linear_blocked` on the materialised operand.  GPU tensors only (a CPU tensor raises), None where the kernel
                         does not cover the call: the caller keeps the two `ops.linear_blocked` launches.

The switch is `SWITCHES.encoder_pair` (univs_amd/switches.py; UNIVS_ENCODER_PAIR=0 restores the two launches and the `src + pos` tensor the
previous layer's FFN kernel writes for them): modeling/pixel_decoder/msdeformattn.py reads it.
"""
import torch

from . import _lib, ops


# fewest rows at which `ops.linear_blocked` answers (csrc/gemm_plan.h resident_covered: 64 tiles of 32 rows): below it the encoder layer
# is on the standard-layout MSDeformAttn operators, with or without the switch
HEAD_MAJOR_MIN_ROWS = 63 * 32 + 1


def linear_pair_blocked(x, add, weight_a, bias_a, col_block_a, weight_b, bias_b, col_block_b):
    """x [B, rows, K], add [1, rows, K] (or [rows, K]) ->
    (F.linear(x, weight_a, bias_a) as [B, N_a / col_block_a, rows, col_block_a],
     F.linear(x + add, weight_b, bias_b) as [B, N_b / col_block_b, rows, col_block_b]), float32 on x's device and current stream, the
    column-blocked layout of `ops.linear_blocked`; None where the entry does not cover the call (include/univs_encoder_hip.h states what it
    does) or the weights' split images are switched off (SWITCHES.resident_presplit, six-product arithmetic)."""
    name = "linear_pair_blocked"
    ops._inference_only(name, x, add, weight_a, weight_b)
    if x.dim() != 3 or add.dim() not in (2, 3) or (add.dim() == 3 and add.shape[0] != 1) or tuple(add.shape[-2:]) != tuple(x.shape[1:]):
        raise RuntimeError(f"{name}: x [B, rows, K] and add [1, rows, K], got {tuple(x.shape)} and {tuple(add.shape)}")
    B, rows, K = (int(v) for v in x.shape)
    tensors = [t for t in (x, add, weight_a, bias_a, weight_b, bias_b) if t is not None]
    if any(t.dtype != torch.float32 for t in tensors) or weight_a.dim() != 2 or weight_b.dim() != 2 or weight_a.shape[1] != K or weight_b.shape[1] != K:
        return None
    x, add = x.contiguous(), add.contiguous()
    ops._require_gpu(name, x, add, weight_a, weight_b)
    Na, Nb, ca, cb = int(weight_a.shape[0]), int(weight_b.shape[0]), int(col_block_a), int(col_block_b)
    if (B < 1 or rows < 1 or ca < 4 or cb < 4 or ca % 4 or cb % 4 or Na % ca or Nb % cb or K != 256
            or not ops._resident_presplit(weight_a, K) or not ops._resident_presplit(weight_b, K)):
        return None
    for b, n in ((bias_a, Na), (bias_b, Nb)):
        if b is not None and (tuple(b.shape) != (n,) or not b.is_cuda or not b.is_contiguous()):
            raise RuntimeError(f"{name}: a bias must be contiguous float32 [N] on the GPU")
    (wpa, wia), (wpb, wib) = ops.presplit_weights(weight_a), ops.presplit_weights(weight_b)
    ya = torch.empty((B, Na // ca, rows, ca), dtype=torch.float32, device=x.device)
    yb = torch.empty((B, Nb // cb, rows, cb), dtype=torch.float32, device=x.device)
    ok = ops._call(name, _lib.load().univs_encoder_linear_pair_presplit_f32, x, ops._ptr(x), ops._ptr(add), rows, ops._ptr(wpa), ops._ptr(wia),
                   ops._opt(bias_a), Na, ca, ops._ptr(ya), ops._ptr(wpb), ops._ptr(wib), ops._opt(bias_b), Nb, cb, ops._ptr(yb), B * rows, K, rows)
    return (ya, yb) if ok else None
