"""Wrappers of the sixteenth header (include/univs_seam_hip.h): the seams of a post-norm decoder layer -- two few-rows kernels of which
the second reads nothing but the first one's output, in ONE launch.  They go through `ops._call` like every wrapper and answer as
`ops.small_linear` / `ops.small_mlp` do: None where the call is not covered (CPU tensors, autograd, other shapes), and the caller keeps
the separate launches.  Every result has the bits of the launches it replaces (tests/test_decoder_seams_gpu.py).

  small_seam      norm(residual + out_proj(x)) and the next sub-layer's first Linear on it (`ops.small_seam` is this function)
  small_mlp_seam  `ops.small_mlp` with the FFN's residual LayerNorm in front of the chain and / or the next layer's cross-attention query
                  projection beside it (`ops.small_mlp(..., pre_ln=, side=)` comes here)
"""
import ctypes

import torch

from . import _lib, ops


def _whole_f32(w, shape=None):
    return (w.dtype == torch.float32 and w.is_cuda and w.dim() == 2 and w._base is None and w.is_contiguous()
            and (shape is None or tuple(w.shape) == shape))


def _vec_f32(b, n):
    return b is None or (b.dtype == torch.float32 and b.is_cuda and tuple(b.shape) == (n,) and b.is_contiguous())


def small_seam(x, weight_a, bias_a, residual, ln, weight_b, bias_b=None, rows=None, add=None, relu=False, add_features=0):
    """t = LayerNorm(residual + x weight_a^T + bias_a) and y = act((t [+ add]) weight_b[rows]^T + bias_b[rows]) in ONE launch
    (include/univs_seam_hip.h: univs_small_seam_presplit_f32; csrc/small_linear.hip: small_seam_kernel) -> (t, y), bit for bit
    `t = ops.small_linear(x, weight_a, bias_a, residual=residual, ln=ln)` and
    `y = ops.small_linear(t, weight_b, bias_b, rows=rows, x_add=add, relu=relu, add_features=add_features)`.
    x [..., 256]; weight_a [256, 256]; `ln` = (weight, bias, eps); weight_b [Nw, 256] whole, `rows` = (first, count) with count % 256 == 0;
    `add` of t's shape.  None where not covered: the caller keeps the two launches."""
    K = x.shape[-1]
    M = x.numel() // max(K, 1)
    if (not x.is_cuda or x.dtype != torch.float32 or K != 256 or M < 1 or M > ops.SMALL_LINEAR_MAX_ROWS or ln is None
            or not _whole_f32(weight_a, (256, 256)) or not _whole_f32(weight_b) or weight_b.shape[1] != 256
            or ops.needs_grad(x, weight_a, bias_a, residual, weight_b, bias_b, add)):
        return None
    Nwb = int(weight_b.shape[0])
    f_off, Nb = (0, Nwb) if rows is None else (int(rows[0]), int(rows[1]))
    if (Nb < 256 or Nb % 256 != 0 or f_off < 0 or f_off % 4 != 0 or f_off + Nb > Nwb or add_features < 0 or add_features % 32 != 0
            or not _vec_f32(bias_a, 256) or not _vec_f32(bias_b, Nwb)):
        return None
    if (residual is None or residual.dtype != torch.float32 or not residual.is_cuda or residual.numel() != M * 256 or residual.shape[-1] != 256):
        return None
    if add is not None and (add.dtype != torch.float32 or not add.is_cuda or tuple(add.shape) != tuple(x.shape)):
        return None
    triple = ops._ln_triple("small_seam", ln, 256, False)
    if triple is None:
        return None
    lw, lb, leps = triple
    x2 = x.contiguous().view(M, K)
    r = residual.contiguous()
    ad = add.contiguous() if add is not None else None
    t = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    y = torch.empty(tuple(x.shape[:-1]) + (Nb,), dtype=torch.float32, device=x.device)
    wpa, wia = ops.presplit_weights(weight_a)
    wpb, wib = ops.presplit_weights(weight_b)
    ok = ops._call("small_seam", _lib.load().univs_small_seam_presplit_f32, x2, ops._ptr(x2), ops._ptr(wpa), ops._ptr(wia), ops._opt(bias_a),
                   ops._ptr(r), ops._opt(lw), ops._opt(lb), leps, ops._ptr(t), ops._opt(ad), ops._ptr(wpb), ops._ptr(wib), ops._opt(bias_b),
                   Nwb, f_off, M, K, 256, Nb, 1 if relu else 0, int(add_features), ops._ptr(y))
    return (t, y) if ok else None


def small_mlp_seam(x, layers_, in_ln=None, want_normed=False, transpose01=False, pre_ln=None, side=None):
    """`ops.small_mlp(x', layers_, in_ln, want_normed, transpose01)` in ONE launch with what stands around it at the end of a decoder layer
    (include/univs_seam_hip.h: univs_small_mlp_seam_presplit_f32; csrc/small_linear.hip: small_chain_kernel):
      pre_ln = (residual, weight, bias, eps): x' = ops.layer_norm(x, weight, bias, eps, residual=residual), bit for bit, and x' is returned;
               without it x' = x.
      side = (weight [Nw, 256], bias [Nw] | None, rows = (first, 256) | None, add | None): also returns
             ops.small_linear(x', weight, bias, rows=rows, x_add=add), bit for bit.
    Returns the tuple (y[, x_normed][, x'][, side_y]) -- the extras in this order, each only where asked for -- or None where not covered."""
    K = x.shape[-1]
    M = x.numel() // max(K, 1)
    n = len(layers_)
    if (not x.is_cuda or x.dtype != torch.float32 or K != 256 or M < 1 or M > ops.SMALL_LINEAR_MAX_ROWS or n < 1 or n > 3
            or (transpose01 and x.dim() != 3) or (want_normed and in_ln is None)):
        return None
    for w, b, _ in layers_:
        if not _whole_f32(w, (256, 256)) or not _vec_f32(b, 256) or ops.needs_grad(x, w, b):
            return None
    triple = ops._ln_triple("small_mlp", in_ln, 256, False)
    if triple is None:
        return None
    lw, lb, leps = triple
    x2 = x.contiguous().view(M, K)
    pres = pw = pb = xo = None
    peps = 0.0
    if pre_ln is not None:
        pres, pw, pb, peps = pre_ln
        if (pw is None or pb is None or pres is None or not _vec_f32(pw, 256) or not _vec_f32(pb, 256) or pres.dtype != torch.float32
                or not pres.is_cuda or tuple(pres.shape) != tuple(x.shape) or ops.needs_grad(pres, pw, pb)):
            return None
        pres = pres.contiguous()
        xo = torch.empty_like(x2)
    sw = sb = sa = swp = swi = sy = None
    s_nw = s_off = 0
    if side is not None:
        sw, sb, srows, sa = side
        if not _whole_f32(sw) or sw.shape[1] != 256:
            return None
        s_nw = int(sw.shape[0])
        s_off, s_n = (0, s_nw) if srows is None else (int(srows[0]), int(srows[1]))
        if (s_n != 256 or s_off < 0 or s_off % 4 != 0 or s_off + 256 > s_nw or s_nw % 4 != 0 or not _vec_f32(sb, s_nw) or ops.needs_grad(sw, sb, sa)
                or (sa is not None and (sa.dtype != torch.float32 or not sa.is_cuda or tuple(sa.shape) != tuple(x.shape)))):
            return None
        sa = sa.contiguous() if sa is not None else None
        swp, swi = ops.presplit_weights(sw)
        sy = torch.empty_like(x2)
    oshape = (x.shape[1], x.shape[0], 256) if transpose01 else tuple(x.shape[:-1]) + (256,)
    y = torch.empty(oshape, dtype=torch.float32, device=x.device)
    xn = torch.empty_like(x2) if want_normed else None
    P3, I3 = ctypes.c_void_p * 3, ctypes.c_int * 3
    split = [ops.presplit_weights(w) for w, _, _ in layers_]
    wp = P3(*([ops._ptr(s_[0]) for s_ in split] + [None] * (3 - n)))
    wi = P3(*([ops._ptr(s_[1]) for s_ in split] + [None] * (3 - n)))
    bs = P3(*([ops._opt(b) for _, b, _ in layers_] + [None] * (3 - n)))
    rl = I3(*([1 if r else 0 for _, _, r in layers_] + [0] * (3 - n)))
    ok = ops._call("small_mlp", _lib.load().univs_small_mlp_seam_presplit_f32, x2, ops._ptr(x2), ops._opt(pres), ops._opt(pw), ops._opt(pb),
                   float(peps), ops._opt(xo), ops._opt(sa), ops._opt(swp), ops._opt(swi), ops._opt(sb), s_nw, s_off, ops._opt(sy), n, wp, wi, bs, rl,
                   ops._opt(lw), ops._opt(lb), leps, ops._opt(xn), M, int(x.shape[1]) if transpose01 else 0, ops._ptr(y))
    if not ok:
        return None
    out = [y]
    if want_normed:
        out.append(xn.view(x.shape))
    if pre_ln is not None:
        out.append(xo.view(x.shape))
    if side is not None:
        out.append(sy.view(x.shape))
    return tuple(out)
