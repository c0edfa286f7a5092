"""The per-frame pair table of a video panoptic evaluation: counts[t, g, p] = the pixels of frame t whose ground-truth segment id is
gt_ids[g] and whose predicted segment id is pred_ids[p].  Everything VPQ and STQ need is a sum over these tables (vps.py).

  panoptic_pair_counts   the HIP kernel (csrc/pair_count.hip) behind `ops._call`: GPU tensors only, None where it does not cover
  pair_counts_aten       the same table from torch.searchsorted + bincount on any device: the fallback, the yardstick, the CPU path
  pair_counts            the kernel on GPU tensors where it covers the call, else the ATen formulation

A map is uint8 [T, H, W, 3] (the decoded panoptic PNG, id = R + 256 G + 65536 B) or int32 [T, H, W]; the two sides may differ.  The id
tables are ascending and unique.  Row G / column P of a table collects the ids that are not listed; first_unknown [T, 2] names the
largest such id of each frame's ground truth / prediction (-1: none that is >= 0).

The wrapper lives here and not in ops.py: its launch is outside the model's forward pass.  Prologue, launch and dispatch are _counts.py's,
shared with vss_counts.py and davis_counts.py; the contract of the three is pinned in tests/test_eval_counts_contract_cpu.py.
"""
import torch

from .. import ops
from . import _counts

MAX_IDS = 1024        # csrc/pair_count.hip: PAIR_MAX_IDS
MAX_CELLS = 16384     # PAIR_MAX_CELLS: (G + 1)(P + 1), the LDS histogram


def _check_map(name, side, x):
    if x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3:
        return True
    if x.dtype == torch.int32 and x.dim() == 3:
        return False
    raise RuntimeError(f"{name}: {side} must be uint8 [T, H, W, 3] or int32 [T, H, W], got {x.dtype} {tuple(x.shape)}")


def _check(name, gt, pred, gt_ids, pred_ids):
    g_rgb, p_rgb = _check_map(name, "gt", gt), _check_map(name, "pred", pred)
    if tuple(gt.shape[:3]) != tuple(pred.shape[:3]) or 0 in gt.shape[:3]:
        raise RuntimeError(f"{name}: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} do not cover the same non-empty [T, H, W]")
    if gt_ids.dim() != 1 or pred_ids.dim() != 1 or gt_ids.numel() == 0 or pred_ids.numel() == 0:
        raise RuntimeError(f"{name}: the id tables must be non-empty 1-d")
    return g_rgb, p_rgb


def panoptic_pair_counts(gt, pred, gt_ids, pred_ids):
    """(counts int32 [T, G + 1, P + 1], first_unknown int32 [T, 2]) from csrc/pair_count.hip on the tensors' device and current stream;
    None where the kernel does not cover the call (G or P > 1024, (G + 1)(P + 1) > 16384, T > 65535): the caller keeps
    `pair_counts_aten`.  CPU tensors raise, as in every wrapper of ops.py."""
    name = "panoptic_pair_counts"
    g_rgb, p_rgb = _counts.admit(name, gt, pred, _check, gt_ids, pred_ids)
    T, H, W = (int(v) for v in gt.shape[:3])
    G, P = int(gt_ids.numel()), int(pred_ids.numel())
    if G > MAX_IDS or P > MAX_IDS or (G + 1) * (P + 1) > MAX_CELLS or T > 65535 or H * W >= 2 ** 31:
        return None
    gt, pred = gt.contiguous(), pred.contiguous()
    gi = gt_ids.to(device=gt.device, dtype=torch.int32).contiguous()
    pi = pred_ids.to(device=gt.device, dtype=torch.int32).contiguous()
    counts = torch.zeros((T, G + 1, P + 1), dtype=torch.int32, device=gt.device)
    unknown = torch.full((T, 2), -1, dtype=torch.int32, device=gt.device)
    return _counts.launch(name, "univs_panoptic_pair_counts", gt, (counts, unknown), ops._ptr(gt), int(g_rgb), ops._ptr(pred), int(p_rgb),
                          T, H, W, ops._ptr(gi), G, ops._ptr(pi), P)


def _flat_ids(x, rgb):
    if rgb:
        x = x.to(torch.int64)
        x = x[..., 0] + 256 * x[..., 1] + 65536 * x[..., 2]
    return x.reshape(x.shape[0], -1).to(torch.int64)


def _table_index(ids, table):
    """(index of each id in the ascending table, len(table) where absent; the ids that are absent, -1 elsewhere)"""
    n = int(table.numel())
    pos = torch.searchsorted(table, ids).clamp_(max=n - 1)
    found = table[pos] == ids
    return torch.where(found, pos, torch.full_like(pos, n)), torch.where(found, torch.full_like(ids, -1), ids)


def pair_counts_aten(gt, pred, gt_ids, pred_ids, with_unknown=False):
    """counts int32 [T, G + 1, P + 1] (and first_unknown int32 [T, 2] with `with_unknown`) on the tensors' device, CPU or GPU."""
    g_rgb, p_rgb = _check("pair_counts_aten", gt, pred, gt_ids, pred_ids)
    T = int(gt.shape[0])
    gtab = gt_ids.to(device=gt.device, dtype=torch.int64).contiguous()
    ptab = pred_ids.to(device=gt.device, dtype=torch.int64).contiguous()
    G, P = int(gtab.numel()), int(ptab.numel())
    gi, gu = _table_index(_flat_ids(gt, g_rgb), gtab)
    pi, pu = _table_index(_flat_ids(pred.to(gt.device), p_rgb), ptab)
    cells = (G + 1) * (P + 1)
    key = gi * (P + 1) + pi + torch.arange(T, device=gt.device, dtype=torch.int64)[:, None] * cells
    counts = torch.bincount(key.reshape(-1), minlength=T * cells).reshape(T, G + 1, P + 1).to(torch.int32)
    if not with_unknown:
        return counts
    unknown = torch.stack([gu.amax(dim=1), pu.amax(dim=1)], dim=1).clamp_(min=-1).to(torch.int32)
    return counts, unknown


def pair_counts(gt, pred, gt_ids, pred_ids):
    """(counts, first_unknown): the kernel on GPU tensors where it covers the call, else the ATen formulation."""
    return _counts.kernel_else_aten(panoptic_pair_counts, lambda *a: pair_counts_aten(*a, with_unknown=True), gt, pred, gt_ids, pred_ids)
