"""Wrappers of the third header (include/univs_fused_hip.h): consumers that apply, while they load their operand, a transform that
would otherwise be a launch and a tensor of its own.  They go through `ops._call` like every wrapper: GPU tensors only (a CPU tensor
raises), None where the kernel does not cover the call -- the caller then keeps the separate launches.

  conv1x1_fused   the pixel decoder's 1 x 1 convolutions on an NCHW or a channels-last operand (a Swin stage output is a channels-last
                  VIEW of its token tensor: no transpose), optionally with relu(GroupNorm(x)) applied to the operand from the pairs
                  of `ops.group_norm_affine` (the mask-feature convolution behind the FPN output convolution: no normalised tensor)
  attention_out_proj  the attention core's partial results per key segment + the out-projection (residual, LayerNorm) that merges them
                  while it stages its operand: `ops.small_linear(ops.cross_attention(...), ...)` without the merge launch
"""
import ctypes

import torch

from . import _lib, ops
from .switches import SWITCHES


def conv1x1_fused(x, weight, bias=None, affine=None):
    """F.conv2d(x', weight [Cout, Cin, 1, 1], bias) -> contiguous NCHW float32, x [T, Cin, H, W] either contiguous or contiguous in
    torch.channels_last (read in place, never copied); x' = x, or with `affine` ([T * Cin, 2] from ops.group_norm_affine(x, ...))
    x' = relu(group_norm(x)).  Bit-identical to ops.conv1x1 on the contiguous (and, with `affine`, normalised) tensor.
    None where not covered."""
    name = "conv1x1_fused"
    for t in (x, weight, bias, affine):
        if t is not None and not t.is_cuda:
            raise ops._cpu_refusal(name, f"tensor on {t.device}")
    ops._inference_only(name, x, weight, bias, affine)
    if (x.dtype != torch.float32 or weight.dtype != torch.float32 or x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[2:]) != (1, 1)
            or weight.shape[1] != x.shape[1] or SWITCHES.presplit_kmin <= 0):
        return None
    T, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(weight.shape[0])
    if x.is_contiguous():
        channels_last = 0
    elif x.is_contiguous(memory_format=torch.channels_last):
        channels_last = 1
    else:
        return None
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (Cout,) or not bias.is_contiguous()):
        return None
    if affine is not None and (affine.dtype != torch.float32 or tuple(affine.shape) != (T * Cin, 2) or not affine.is_contiguous()):
        raise RuntimeError(f"{name}: affine must be contiguous float32 [T * Cin, 2] = {(T * Cin, 2)}, got {affine.dtype} {tuple(affine.shape)}")
    y = torch.empty((T, Cout, H, W), dtype=torch.float32, device=x.device)
    wp, winv = ops.presplit_weights(weight)
    ok = ops._call(name, _lib.load().univs_conv1x1_fused_presplit_f32, x, ops._ptr(x), channels_last, ops._opt(affine), ops._ptr(wp),
                   ops._ptr(winv), ops._opt(bias), T, Cin, Cout, H, W, ops._ptr(y))
    return y if ok else None


def attention_out_proj(q, k, v, mask, num_heads, scale, weight, bias=None, residual=None, ln=None):
    """ops.small_linear(ops.cross_attention(q, k, v, mask, num_heads, scale), weight, bias, residual=residual, ln=ln), bit for bit, in two
    launches instead of three: the attention output [L, N, E] is never written (include/univs_fused_hip.h).  Arguments as those two
    wrappers'; `weight` [E_out, E] whole (its split is cached per tensor).  None where either kernel does not cover the call."""
    name = "attention_out_proj"
    for t in (q, k, v, weight, bias, residual):
        if t is not None and not t.is_cuda:
            raise ops._cpu_refusal(name, f"tensor on {t.device}")
    ops._inference_only(name, q, k, v, weight, bias, residual)
    args = ops._cross_attention_args(q, k, v, mask, num_heads)
    if args is None or weight.dtype != torch.float32 or weight.dim() != 2:
        return None
    q, k, v, mask, flags, gen, L, S, N, H, ldq, ldk, ldv = args
    Nw, M = int(weight.shape[0]), L * N
    if weight.shape[1] != 32 * H or 32 * H > ops.SMALL_LINEAR_MAX_K or M > ops.SMALL_LINEAR_MAX_ROWS or Nw % 16 != 0 or (ln is not None and Nw != 256):
        return None
    r = None
    if residual is not None:
        if residual.dtype != torch.float32 or residual.numel() != M * Nw or residual.shape[-1] != Nw:
            return None
        r = residual.contiguous()
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (Nw,) or not bias.is_contiguous()):
        return None
    triple = ops._ln_triple(name, ln, Nw, False)
    if triple is None:
        return None
    lw, lb, leps = triple
    lib = _lib.load()
    ws = torch.empty(int(lib.univs_cross_attention_workspace(L, S, N, H)), dtype=torch.float32, device=q.device)
    plan = ctypes.c_int(0)
    if not ops._call(name, lib.univs_cross_attention_partials_f32, q, ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._opt(mask), ops._opt(flags),
                     gen, L, S, N, H, 32, ldq, ldk, ldv, float(scale), ops._ptr(ws), ctypes.byref(plan)):
        return None
    y = torch.empty((L, N, Nw), dtype=torch.float32, device=q.device)
    wp, winv = ops.presplit_weights(weight)
    ok = ops._call(name, lib.univs_small_linear_merged_presplit_f32, q, ops._ptr(ws), ws.numel(), plan.value, L, N, H, ops._ptr(wp),
                   ops._ptr(winv), ops._opt(bias), Nw, 0, ops._opt(r), ops._opt(lw), ops._opt(lb), leps, Nw, ops._ptr(y))
    if not ok:
        raise _lib.UnivsHipError(f"{name}: the out-projection refused the plan {plan.value} of L={L} N={N} H={H} after the partials ran")
    return y
