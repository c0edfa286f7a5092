"""The counts of a VSPW evaluation, per video: everything mIoU and the video consistency scores VC8 / VC16 need (vss.py).

  vss_video_counts   the HIP kernel (csrc/vss_count.hip) behind `ops._call`: GPU tensors only, None where it does not cover
  vss_counts_aten    the same three tensors from torch ops on any device: the fallback, the yardstick, the CPU path
  vss_counts         the kernel on GPU tensors where it covers the call, else the ATen formulation

gt is uint8 [T, H, W], the raw VSPW mask values (0 = "others", 1..124, 255 = void), pred uint8 [T, H, W], the bytes of the prediction
PNGs.  The ground truth is mapped as the reference's `map_category_id` does (0 -> 255, v -> v - 1, 254 -> 255 in uint8: raw 0 and raw
255 are one label afterwards); every comparison is on mapped values.  All three return

  confusion int32 [C, C]     cell C g + p counts the pixels with mapped gt g < C and prediction byte p, not clamped: p >= C lands in a
                             later row, as `np.bincount(...).reshape` puts it (eval_utils_vss.py:96-105)
  windows   int32 [T, 2, 2]  [i, n in (8, 16), (den, num)]: the pixels whose mapped gt is equal over frames i .. i + n - 1, and those whose
                             prediction is equal over them too (`get_common`); zero where the window does not fit
  overflow  int32 [1]        the largest cell >= C C (it is not counted: the reference's reshape fails there), -1 when there is none
"""
import torch

from .. import ops
from . import _counts

MAX_CELLS = 16384     # csrc/vss_count.hip: VSS_MAX_CELLS, C C (the LDS histogram)
MAX_FRAMES = 1024     # VSS_MAX_FRAMES: the window records in LDS
CLIP_NUMS = (8, 16)


def _check(name, gt, pred, num_classes):
    _counts.check_uint8_pair(name, gt, pred)
    if int(num_classes) < 1:
        raise RuntimeError(f"{name}: num_classes {num_classes}")


def vss_video_counts(gt, pred, num_classes):
    """(confusion, windows, overflow) from csrc/vss_count.hip on the tensors' device and current stream; None where the kernel does not
    cover the call (C C > 16384, T > 1024, T H W >= 2^31 - 4): the caller keeps `vss_counts_aten`.  CPU tensors raise, as in every
    wrapper of ops.py."""
    name = "vss_video_counts"
    _counts.admit(name, gt, pred, _check, num_classes)
    T, H, W = (int(v) for v in gt.shape)
    C = int(num_classes)
    if C * C > MAX_CELLS or T > MAX_FRAMES or T * H * W >= 2 ** 31 - 4:
        return None
    gt, pred = gt.contiguous(), pred.contiguous()
    confusion = torch.zeros((C, C), dtype=torch.int32, device=gt.device)
    windows = torch.zeros((T, 2, 2), dtype=torch.int32, device=gt.device)
    overflow = torch.full((1,), -1, dtype=torch.int32, device=gt.device)
    return _counts.launch(name, "univs_vss_video_counts", gt, (confusion, windows, overflow), ops._ptr(gt), ops._ptr(pred), T, H, W, C)


def map_category_id(gt):
    """The reference's map (vss_evaluation.py:226-232) on a uint8 tensor, out of place."""
    m = gt - 1                                                       # uint8: 0 -> 255, 255 -> 254
    return torch.where(m == 254, torch.full_like(m, 255), m)


def vss_counts_aten(gt, pred, num_classes):
    """(confusion, windows, overflow) on the tensors' device, CPU or GPU."""
    _check("vss_counts_aten", gt, pred, num_classes)
    C, T = int(num_classes), int(gt.shape[0])
    pred = pred.to(gt.device)
    g = map_category_id(gt).reshape(T, -1)
    p = pred.reshape(T, -1)
    keep = g < C
    cell = C * g[keep].to(torch.int64) + p[keep].to(torch.int64)
    beyond = cell >= C * C
    overflow = cell[beyond].max().reshape(1).to(torch.int32) if bool(beyond.any()) else torch.full((1,), -1, dtype=torch.int32, device=gt.device)
    confusion = torch.bincount(cell[~beyond], minlength=C * C).reshape(C, C).to(torch.int32)
    windows = torch.zeros((T, 2, 2), dtype=torch.int32, device=gt.device)
    if T > 1:
        same_g = g[1:] == g[:-1]                                     # [T - 1, H W]: frame t + 1 against frame t
        same_b = same_g & (p[1:] == p[:-1])
        zero = torch.zeros((1, g.shape[1]), dtype=torch.int32, device=gt.device)
        run_g = torch.cat([zero, torch.cumsum(same_g.to(torch.int32), dim=0, dtype=torch.int32)])
        run_b = torch.cat([zero, torch.cumsum(same_b.to(torch.int32), dim=0, dtype=torch.int32)])
        for k, n in enumerate(CLIP_NUMS):
            if T >= n:                                               # window i is common iff its n - 1 steps all are
                windows[:T - n + 1, k, 0] = ((run_g[n - 1:] - run_g[:T - n + 1]) == n - 1).sum(dim=1)
                windows[:T - n + 1, k, 1] = ((run_b[n - 1:] - run_b[:T - n + 1]) == n - 1).sum(dim=1)
    return confusion, windows, overflow


def vss_counts(gt, pred, num_classes):
    """(confusion, windows, overflow): the kernel on GPU tensors where it covers the call, else the ATen formulation."""
    return _counts.kernel_else_aten(vss_video_counts, vss_counts_aten, gt, pred, num_classes)
