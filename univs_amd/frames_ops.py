"""Wrapper of the eighth header (include/univs_frames_hip.h): the test-time resize of decoded frames.

  resize_frames_u8     the HIP kernel (csrc/frame_resize.hip) behind `ops._call`: GPU tensors only (a CPU tensor raises), None where
                       the kernel does not cover the call

frames is uint8 [T, Hi, Wi, 3] (HWC, as an image file decodes); the result is uint8 [T, 3, Ho, Wo], every frame
`PIL.Image.resize((Wo, Ho), BILINEAR)` bit for bit (data/resize_rule.py states the rule and is the yardstick; the host path of
data/mapper.py is Pillow itself).  The kernel takes its coefficient tables as arguments; they are computed on the host in float64
(data/resize_rule.py: `resize_tables`) and uploaded once per (n_in, n_out, device).
"""
from collections import OrderedDict

import torch

from . import _lib, ops
from .data.resize_rule import KSIZE_MAX, axis_ksize, resize_tables

_TABLES = OrderedDict()                                              # (n_in, n_out, device) -> (first, count, coef) on the device
_TABLES_MAX = 16


def _tables(n_in, n_out, device):
    key = (n_in, n_out, str(device))
    hit = _TABLES.get(key)
    if hit is not None:
        _TABLES.move_to_end(key)
        return hit
    hit = tuple(torch.from_numpy(a).to(device) for a in resize_tables(n_in, n_out))
    _TABLES[key] = hit
    while len(_TABLES) > _TABLES_MAX:
        _TABLES.popitem(last=False)
    return hit


def resize_frames_u8(frames, out_hw, bgr=False):
    """uint8 [T, 3, Ho, Wo] from csrc/frame_resize.hip on the frames' device and current stream; `bgr` swaps channels 0 and 2 on the way
    (RGB files, a model with INPUT.FORMAT "BGR").  None where the kernel does not cover the sizes (include/univs_frames_hip.h states
    them: a down-scale beyond 4 on either axis, or 2^31 bytes): the caller resizes with Pillow.  CPU tensors raise, as in every wrapper
    of ops.py."""
    name = "resize_frames_u8"
    ops._require_gpu(name, frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or 0 in frames.shape:
        raise RuntimeError(f"{name}: uint8 [T, H, W, 3] frames, got {frames.dtype} {tuple(frames.shape)}")
    Ho, Wo = (int(v) for v in out_hw)
    if Ho < 1 or Wo < 1:
        raise RuntimeError(f"{name}: out_hw {tuple(out_hw)}")
    T, Hi, Wi, _ = (int(v) for v in frames.shape)
    ksx, ksy = axis_ksize(Wi, Wo), axis_ksize(Hi, Ho)
    if ksx > KSIZE_MAX or ksy > KSIZE_MAX or 3 * T * max(Hi * Wi, Ho * Wo) >= 2 ** 31:
        return None                                                  # (the entry's answer, without building tables it would not read)
    tx = _tables(Wi, Wo, frames.device) if Wi != Wo else (None, None, None)
    ty = _tables(Hi, Ho, frames.device) if Hi != Ho else (None, None, None)
    out = torch.empty((T, 3, Ho, Wo), dtype=torch.uint8, device=frames.device)
    ok = ops._call(name, _lib.load().univs_resize_frames_u8, frames, ops._ptr(frames), T, Hi, Wi, Ho, Wo, *(ops._opt(t) for t in tx), ksx,
                   *(ops._opt(t) for t in ty), ksy, int(bool(bgr)), ops._ptr(out))
    return out if ok else None
