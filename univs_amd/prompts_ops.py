"""Wrapper of the ninth header (include/univs_prompts_hip.h): the first-frame masks of a VOS video at the model's input size.

  resize_rle_masks_u8  the HIP kernel (csrc/mask_prompt_resize.hip) behind `ops._call`: GPU tensors only (a CPU tensor raises), None
                       where the kernel does not cover the call

runs is the `Runs` of evaluation/vis_counts.py (`runs_from_rles`) for the N annotated masks of a video, all of one size; the result is
(uint8 [N, Ho, Wo], int32 [N, 4]): every mask `PIL.Image.resize((Wo, Ho), NEAREST)` byte for byte (data/resize_rule.py states the rule
and is the yardstick; the host path of data/vos_mapper.py is Pillow itself) and its box {x0, y0, x1 + 1, y1 + 1}, zeros for an empty or
absent mask.  The kernel takes its two index tables as arguments; they are computed on the host in float64 (data/resize_rule.py:
`nearest_table`) and uploaded once per (n_in, n_out, device).
"""
from collections import OrderedDict

import torch

from . import _lib, ops
from .data.resize_rule import nearest_table

_TABLES = OrderedDict()                                              # (n_in, n_out, device) -> int32 [n_out] on the device
_TABLES_MAX = 16


def _table(n_in, n_out, device):
    key = (n_in, n_out, str(device))
    hit = _TABLES.get(key)
    if hit is not None:
        _TABLES.move_to_end(key)
        return hit
    hit = torch.from_numpy(nearest_table(n_in, n_out)).to(device)
    _TABLES[key] = hit
    while len(_TABLES) > _TABLES_MAX:
        _TABLES.popitem(last=False)
    return hit


def resize_rle_masks_u8(runs, in_hw, out_hw):
    """(masks uint8 [N, Ho, Wo], boxes int32 [N, 4]) from csrc/mask_prompt_resize.hip on the runs' device and current stream.  None
    where the kernel does not cover the sizes (include/univs_prompts_hip.h states them: H W, the boundaries or N Ho Wo beyond 2^31):
    the caller resizes with Pillow.  CPU tensors raise, as in every wrapper of ops.py."""
    name = "resize_rle_masks_u8"
    bounds, starts = runs.bounds, runs.starts
    ops._require_gpu(name, bounds, starts)
    if bounds.dtype != torch.int32 or starts.dtype != torch.int32 or bounds.dim() != 1 or starts.dim() != 1 or starts.numel() < 1:
        raise RuntimeError(f"{name}: int32 vectors bounds and starts [N + 1], got {bounds.dtype} {tuple(bounds.shape)} and "
                           f"{starts.dtype} {tuple(starts.shape)}")
    (H, W), (Ho, Wo) = (int(v) for v in in_hw), (int(v) for v in out_hw)
    if H < 1 or W < 1 or Ho < 1 or Wo < 1:
        raise RuntimeError(f"{name}: in_hw {tuple(in_hw)} out_hw {tuple(out_hw)}")
    N = starts.numel() - 1
    if H * W >= 2 ** 31 or N * Ho * Wo >= 2 ** 31:
        return None                                                  # (the entry's answer, without building tables it would not read)
    masks = torch.empty((N, Ho, Wo), dtype=torch.uint8, device=bounds.device)
    boxes = torch.empty((N, 4), dtype=torch.int32, device=bounds.device)
    if N == 0:
        return masks, boxes
    ty, tx = _table(H, Ho, bounds.device), _table(W, Wo, bounds.device)
    some = bounds if bounds.numel() else bounds.new_zeros(1)         # (every mask absent: no NULL pointer)
    ok = ops._call(name, _lib.load().univs_resize_rle_masks_u8, bounds, ops._ptr(some), ops._ptr(starts), bounds.numel(), N, H, W,
                   ops._ptr(ty), ops._ptr(tx), Ho, Wo, ops._ptr(masks), ops._ptr(boxes))
    return (masks, boxes) if ok else None
