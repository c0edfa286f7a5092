"""Wrappers of the fifteenth header (include/univs_idmap_hip.h): the prompts of a VOS video from the id maps of its annotation PNGs.

  idmap_census_u8   per frame and value the pixel count and the box at the source size (csrc/idmap_prompts.hip)
  idmap_prompts_u8  the listed objects' masks at the model's input size and their boxes, gathered from the id maps
  upload_prompts    the wrapper's inputs from host arrays: the id maps and the two lists in ONE upload

Both run behind `ops._call`: GPU tensors only (a CPU tensor raises), None where the kernel does not cover the call.
data/idmap_rule.py states both in numpy and is the yardstick.  The prompts kernel takes its two index tables as arguments; they are
computed on the host in float64 (data/resize_rule.py: `nearest_table`) and uploaded once per (n_in, n_out, device), in the cache
prompts_ops.py keeps.
"""
import numpy as np
import torch

from . import _lib, ops
from .prompts_ops import _table


def _check_ids(name, ids):
    ops._require_gpu(name, ids)
    if ids.dtype != torch.uint8 or ids.dim() != 3 or ids.shape[1] < 1 or ids.shape[2] < 1:
        raise RuntimeError(f"{name}: uint8 id maps [F, H, W], got {ids.dtype} {tuple(ids.shape)}")
    return (int(v) for v in ids.shape)


def idmap_census_u8(ids):
    """(count int32 [F, 256], box int32 [F, 256, 4]) of uint8 [F, H, W] on its device and current stream; None beyond F H W < 2^31."""
    name = "idmap_census_u8"
    F, H, W = _check_ids(name, ids)
    if F * H * W >= 2 ** 31:
        return None
    count = torch.empty((F, 256), dtype=torch.int32, device=ids.device)
    box = torch.empty((F, 256, 4), dtype=torch.int32, device=ids.device)
    if F == 0:
        return count, box
    ok = ops._call(name, _lib.load().univs_idmap_census_u8, ids, ops._ptr(ids), F, H, W, ops._ptr(count), ops._ptr(box))
    return (count, box) if ok else None


def idmap_prompts_u8(ids, frame, value, out_hw):
    """(masks uint8 [N, Ho, Wo], boxes int32 [N, 4]): object n is value[n] in frame[n] of ids (int32 [N] each, frame non-decreasing),
    resized as `PIL.Image.resize((Wo, Ho), NEAREST)` resizes its plane.  None where the kernel does not cover the sizes
    (include/univs_idmap_hip.h: F H W or N Ho Wo beyond 2^31): the caller resizes with Pillow.  CPU tensors raise."""
    name = "idmap_prompts_u8"
    ops._require_gpu(name, ids, frame, value)
    F, H, W = _check_ids(name, ids)
    if frame.dtype != torch.int32 or value.dtype != torch.int32 or frame.dim() != 1 or value.shape != frame.shape:
        raise RuntimeError(f"{name}: int32 vectors frame and value [N], got {frame.dtype} {tuple(frame.shape)} and "
                           f"{value.dtype} {tuple(value.shape)}")
    Ho, Wo = (int(v) for v in out_hw)
    N = frame.numel()
    if Ho < 1 or Wo < 1 or (N > 0 and F == 0):
        raise RuntimeError(f"{name}: ids {tuple(ids.shape)} N={N} out_hw {tuple(out_hw)}")
    if F * H * W >= 2 ** 31 or N * Ho * Wo >= 2 ** 31:
        return None                                                  # (the entry's answer, without building tables it would not read)
    masks = torch.empty((N, Ho, Wo), dtype=torch.uint8, device=ids.device)
    boxes = torch.empty((N, 4), dtype=torch.int32, device=ids.device)
    if N == 0:
        return masks, boxes
    ty, tx = _table(H, Ho, ids.device), _table(W, Wo, ids.device)
    ok = ops._call(name, _lib.load().univs_idmap_prompts_u8, ids, ops._ptr(ids), F, H, W, ops._ptr(frame), ops._ptr(value), N, ops._ptr(ty),
                   ops._ptr(tx), Ho, Wo, ops._ptr(masks), ops._ptr(boxes))
    return (masks, boxes) if ok else None


def upload_prompts(idmaps, frame, value, device):
    """(ids uint8 [F, H, W], frame int32 [N], value int32 [N]) on `device` from host arrays, in one copy: the two lists ride in front of
    the id maps' bytes."""
    idmaps = np.ascontiguousarray(idmaps, dtype=np.uint8)
    lists = np.ascontiguousarray(np.stack([np.asarray(frame, np.int32).reshape(-1), np.asarray(value, np.int32).reshape(-1)]))
    n = lists.shape[1]
    packed = torch.from_numpy(np.concatenate([lists.view(np.uint8).reshape(-1), idmaps.reshape(-1)])).to(device)
    lists_d = packed[:8 * n].view(torch.int32)
    return packed[8 * n:].view(idmaps.shape), lists_d[:n], lists_d[n:]
