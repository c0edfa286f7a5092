"""Wrapper of the seventh header (include/univs_swin_hip.h): Swin window attention that computes q, k, v from the tokens itself.

  window_attention_qkv   image-mode window attention on the NORMALISED TOKENS x [B, H*W, C] and the qkv Linear's parameters in ONE launch
                         (csrc/window_attn_qkv.hip): the [B, H*W, 3C] tensor between the two is never written.  The result has the bits of
                         `ops.linear_fused(x, weight, bias)` followed by `ops.window_attention_image(..., mma="f16x3")` where the Linear
                         takes the three-product kernels (2048 rows and more).  GPU tensors only (a CPU tensor raises), None where the
                         kernel does not cover the call: the caller keeps the two launches.

The switch is `SWITCHES.swin_fused_qkv` (univs_amd/switches.py; UNIVS_SWIN_FUSED_QKV): modeling/backbone/swin.py reads it.
"""
import torch

from . import _lib, ops


def window_attention_qkv(x, weight, qkv_bias, bias, shift_mask, H, W, window_size, shift, scale):
    """x [B, H*W, C] float32 tokens in image order, weight [3C, C] and qkv_bias [3C] (or None) of the qkv Linear, bias [nH, ws*ws, ws*ws]
    the relative-position table, shift_mask [nW, ws*ws, ws*ws] (required when shift > 0) -> [B, H*W, C] on x's device and current stream:
    `ops.window_attention_image(linear(x, weight, qkv_bias).view(B, H*W, 3, nH, C // nH), qkv_bias, bias, shift_mask, H, W, window_size,
    shift, scale, mma="f16x3")`.  None where the entry does not cover the call (include/univs_swin_hip.h states what it does: 7 x 7
    windows, head_dim 32, C in {96, 192}, aligned x), the weight is not a whole contiguous tensor (its split image is cached per tensor
    object) or the weights' split images are switched off (SWITCHES.resident_presplit, six-product arithmetic)."""
    name = "window_attention_qkv"
    ops._inference_only(name, x, weight, qkv_bias, bias)
    if x.dim() != 3 or weight.dim() != 2 or bias.dim() != 3:
        raise RuntimeError(f"{name}: x [B, H*W, C], weight [3C, C] and bias [nH, n, n], got {tuple(x.shape)}, {tuple(weight.shape)} and {tuple(bias.shape)}")
    B, L, C = (int(v) for v in x.shape)
    ws, nH = int(window_size), int(bias.shape[0])
    n = ws * ws
    if L != H * W or tuple(weight.shape) != (3 * C, C) or tuple(bias.shape) != (nH, n, n):
        raise RuntimeError(f"{name}: bad shapes")
    tensors = [t for t in (x, weight, qkv_bias, bias, shift_mask) if t is not None]
    if any(t.dtype != torch.float32 for t in tensors):
        return None
    x = x.contiguous()
    ops._require_gpu(name, x, bias)
    if not weight.is_cuda:
        raise ops._cpu_refusal(name, f"tensor on {weight.device}")
    nW = ((H + ws - 1) // ws) * ((W + ws - 1) // ws)
    if shift:
        if shift_mask is None:
            raise RuntimeError(f"{name}: shift > 0 needs the shift mask")
        ops._require_gpu(name, shift_mask)
        if tuple(shift_mask.shape) != (nW, n, n):
            raise RuntimeError(f"{name}: bad shift_mask shape")
    else:
        shift_mask = None
    if qkv_bias is not None:
        ops._require_gpu(name, qkv_bias)
        if tuple(qkv_bias.shape) != (3 * C,):
            raise RuntimeError(f"{name}: bad qkv_bias shape")
    if ws != 7 or C != 32 * nH or C not in (96, 192) or not ops._resident_presplit(weight, C):
        return None
    wp, winv = ops.presplit_weights(weight)
    out = torch.empty((B, L, C), dtype=torch.float32, device=x.device)
    ok = ops._call(name, _lib.load().univs_swin_window_attention_qkv_presplit_f32, x, ops._ptr(x), ops._ptr(wp), ops._ptr(winv), ops._opt(qkv_bias),
                   ops._ptr(bias), ops._opt(shift_mask), B, int(H), int(W), ws, int(shift), nH, C, float(scale), ops._ptr(out))
    return out if ok else None
