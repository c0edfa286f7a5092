"""The counts of a YouTube-VIS evaluation, per video: the per-frame overlap |d_t AND g_t| of every detection and every ground truth,
read off the run-length codes (ytvis.py).  The reference's `iou_seq` (univs/data/datasets/ytvis_api/ytvoseval.py:200-214) is
I / (A_d + A_g - I) with I the sum of the overlaps over the frames and A the summed areas; a `None` frame adds what an empty mask adds.

  runs_from_rles       RLE dicts (compressed strings, uncompressed count lists) and None -> `Runs`, the layout of both sides
  vis_video_overlap    the HIP kernel (csrc/vis_overlap.hip) behind `ops._call`: GPU tensors only, None where it does not cover
  vis_overlap_aten     the same table from torch ops on any device: the fallback, the yardstick, the CPU path
  vis_overlap          the kernel on GPU tensors where it covers the call, else the ATen formulation

`Runs` = (bounds, ones, starts), all int32.  `bounds`: the cumulative column-major run boundaries of all masks back to back; mask m
owns bounds[starts[m] : starts[m + 1]], its run k covers [b_{k-1}, b_k) with b_{-1} = 0, odd runs are foreground, the last boundary is
H W (what `results.mask_run_lengths` has before it takes differences).  `ones[k]`: the foreground pixels of the mask in [0, b_k).
starts[m + 1] == starts[m]: the mask is absent (None).  The masks of a side are object-major: d T + t, g T + t.  All three return
int32 [D, G, T].
"""
from typing import NamedTuple

import numpy as np
import torch

from .. import ops
from . import _counts

MAX_BOUNDS = 16384    # csrc/vis_overlap.hip: VO_MAX_BOUNDS, the boundaries of one ground-truth mask in LDS (128 KB)


class Runs(NamedTuple):
    bounds: torch.Tensor
    ones: torch.Tensor
    starts: torch.Tensor

    @property
    def is_cuda(self):
        return all(x.is_cuda for x in self)

    @property
    def device(self):
        return self.bounds.device

    def to(self, device):
        return Runs(*(x.to(device) for x in self))

    def areas(self):
        """int64 [masks]: the foreground pixels of every mask (0 for an absent one)."""
        s = self.starts.to(torch.int64)
        last = (s[1:] - 1).clamp(min=0)
        a = self.ones.to(torch.int64)[last] if self.ones.numel() else torch.zeros_like(last)
        return torch.where(s[1:] > s[:-1], a, torch.zeros_like(a))


# ---- run-length codes -> Runs ------------------------------------------------------------------------------------------------------------
def _segment_cumsum(v, seg):
    """cumsum of int64 `v` that restarts wherever the non-decreasing `seg` changes."""
    if v.shape[0] == 0:
        return v
    cs = np.cumsum(v)
    first = np.flatnonzero(np.concatenate([[True], seg[1:] != seg[:-1]]))
    base = cs[first] - v[first]
    return cs - np.repeat(base, np.diff(np.concatenate([first, [v.shape[0]]])))


def _string_counts(strings):
    """The run lengths of compressed RLE strings (pycocotools' rleFrString: 5 payload bits and a continuation bit per character, offset
    48, the last character's bit 0x10 is the sign, counts after the third stored as differences to the count two places back), over all
    characters of all strings at once -> (int64 counts back to back, int64 number of counts per string)."""
    raw = [s if isinstance(s, (bytes, bytearray)) else s.encode("ascii") for s in strings]
    c = np.frombuffer(b"".join(raw), dtype=np.uint8).astype(np.int64) - 48
    n_chars = np.array([len(r) for r in raw], dtype=np.int64)
    if c.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(len(raw), np.int64)
    more = (c & 0x20) != 0
    str_end = np.cumsum(n_chars)[n_chars > 0] - 1
    if more[str_end].any():
        raise ValueError("a compressed RLE string ends inside a count")
    first = np.flatnonzero(np.concatenate([[True], ~more[:-1]]))    # the first character of every count
    last = np.concatenate([first[1:], [c.shape[0]]]) - 1
    k = np.arange(c.shape[0]) - np.repeat(first, last - first + 1)   # the character's place inside its count
    if (k > 12).any():
        raise ValueError("a compressed RLE string holds a count of more than 13 characters")
    x = np.add.reduceat((c & 0x1F) << (5 * k), first)                # disjoint bit fields: the sum is the OR
    neg = (c[last] & 0x10) != 0
    x = np.where(neg, x | -(np.int64(1) << np.minimum(5 * (k[last] + 1), 62)), x)
    # which string a count belongs to, and its place there
    sid = np.repeat(np.arange(len(raw)), n_chars)[first]
    per_string = np.bincount(sid, minlength=len(raw))
    pos = np.arange(x.shape[0]) - np.repeat(np.cumsum(per_string) - per_string, per_string)
    # undo the differences: out[j] = x[j] + out[j - 2] for j >= 3, i.e. a running sum along the odd places, and along the even places from 2
    out = x.copy()
    for sel in (np.flatnonzero(pos % 2 == 1), np.flatnonzero((pos % 2 == 0) & (pos >= 2))):
        out[sel] = _segment_cumsum(x[sel], sid[sel])
    return out, per_string


def runs_from_rles(rles, H, W, device=None, video=None):
    """`rles`: one entry per mask -- {"size": [H, W], "counts": str | bytes} (compressed), {"size", "counts": list} (uncompressed) or
    None / an empty entry (absent) -> `Runs` on `device`.  A code whose runs do not sum to H W, or whose size is not the video's, is a
    ValueError that names `video`; a polygon list is a NotImplementedError (pycocotools' rasteriser is not restated here)."""
    what = f"video {video}" if video is not None else "the video"
    hw = int(H) * int(W)
    n = len(rles)
    per_mask = np.zeros(n, np.int64)
    strings, string_at, lists = [], [], {}
    for i, r in enumerate(rles):
        if not r:
            continue
        if isinstance(r, (list, tuple)):
            raise NotImplementedError(f"{what}: mask {i} is a polygon segmentation; only run-length codes are scored")
        if [int(v) for v in r["size"]] != [int(H), int(W)]:
            raise ValueError(f"{what}: mask {i} has size {list(r['size'])}, the video is {[int(H), int(W)]}")
        if isinstance(r["counts"], (list, tuple, np.ndarray)):
            lists[i] = np.asarray(r["counts"], dtype=np.int64).reshape(-1)
            per_mask[i] = lists[i].shape[0]
        else:
            strings.append(r["counts"])
            string_at.append(i)
    if strings:
        flat, per_string = _string_counts(strings)
        per_mask[string_at] = per_string
    starts = np.concatenate([[0], np.cumsum(per_mask)])
    counts = np.zeros(int(starts[-1]), np.int64)
    if strings:
        keep = np.zeros(n, bool)
        keep[string_at] = True
        counts[np.repeat(keep, per_mask)] = flat
    for i, v in lists.items():
        counts[starts[i]:starts[i + 1]] = v
    sid = np.repeat(np.arange(n), per_mask)
    pos = np.arange(counts.shape[0]) - np.repeat(starts[:-1], per_mask)
    bounds = _segment_cumsum(counts, sid)
    ones = _segment_cumsum(np.where(pos % 2 == 1, counts, 0), sid)
    present = np.flatnonzero(per_mask > 0)
    total = bounds[starts[1:][present] - 1]
    if (counts < 0).any() or (total != hw).any():
        bad = int(present[np.flatnonzero(total != hw)[0]]) if (total != hw).any() else int(sid[np.flatnonzero(counts < 0)[0]])
        raise ValueError(f"{what}: the runs of mask {bad} do not cover its {int(H)} x {int(W)} = {hw} pixels")
    if hw >= 2 ** 31 or starts[-1] >= 2 ** 31:
        raise ValueError(f"{what}: {hw} pixels / {int(starts[-1])} runs do not fit 32-bit run boundaries")
    return Runs(*(torch.from_numpy(a.astype(np.int32)).to(device or "cpu") for a in (bounds, ones, starts)))


# ---- the three overlap functions -------------------------------------------------------------------------------------------------------
def _check(name, gt_runs, dt_runs, T, H, W):
    """-> (D, G).  (`gt` first: the order of _counts.admit.)"""
    T = int(T)
    if T < 1 or int(H) < 1 or int(W) < 1:
        raise RuntimeError(f"{name}: T={T} H={H} W={W}")
    n = []
    for side, r in (("gt", gt_runs), ("dt", dt_runs)):
        for x in r:
            if x.dtype != torch.int32 or x.dim() != 1:
                raise RuntimeError(f"{name}: the {side} runs must be int32 vectors, got {x.dtype} {tuple(x.shape)}")
        masks = r.starts.numel() - 1
        if masks < T or masks % T != 0 or r.bounds.numel() != r.ones.numel():
            raise RuntimeError(f"{name}: {masks} {side} masks for T={T}, {r.bounds.numel()} bounds and {r.ones.numel()} ones")
        n.append(masks // T)
    if n[0] * n[1] * T >= 2 ** 31:
        raise RuntimeError(f"{name}: D={n[1]} G={n[0]} T={T}: the table does not fit a 32-bit index")
    return n[1], n[0]


def _padded(x):
    return x if x.numel() else x.new_zeros(1)                        # (a side whose masks are all absent: no NULL pointer)


def vis_video_overlap(dt_runs, gt_runs, T, H, W):
    """inter int32 [D, G, T] from csrc/vis_overlap.hip on the tensors' device and current stream; None where the kernel does not cover the
    call (H W >= 2^31, T > 65535, a ground-truth mask of more than MAX_BOUNDS boundaries): the caller keeps `vis_overlap_aten`.  CPU tensors raise,
    as in every wrapper of ops.py."""
    name = "vis_video_overlap"
    D, G = _counts.admit(name, gt_runs, dt_runs, _check, T, H, W)
    T, H, W = int(T), int(H), int(W)
    cap = int(gt_runs.starts.diff().max()) if gt_runs.starts.numel() > 1 else 0
    if H * W >= 2 ** 31 or cap > MAX_BOUNDS or T > 65535:
        return None
    inter = torch.empty((D, G, T), dtype=torch.int32, device=gt_runs.device)      # every cell is written by the kernel
    dt_runs, gt_runs = Runs(*(x.contiguous() for x in dt_runs)), Runs(*(x.contiguous() for x in gt_runs))
    r = _counts.launch(name, "univs_vis_overlap_counts", gt_runs.bounds, (inter,), ops._ptr(_padded(dt_runs.bounds)), ops._ptr(dt_runs.starts),
                       ops._ptr(_padded(gt_runs.bounds)), ops._ptr(_padded(gt_runs.ones)), ops._ptr(gt_runs.starts), D, G, T, H, W, cap)
    return None if r is None else r[0]


def _dense_frame(runs, t, T, hw):
    """uint8-valued float rows [masks of frame t, H W] of one side: every present mask's runs expanded by one `repeat_interleave`."""
    bounds, _, starts = runs
    starts = starts.to(torch.int64)
    per_mask = starts[1:] - starts[:-1]
    n = per_mask.numel() // T
    mask_of = torch.repeat_interleave(torch.arange(per_mask.numel(), device=bounds.device), per_mask)
    pos = torch.arange(bounds.numel(), device=bounds.device) - starts[:-1][mask_of]
    b = bounds.to(torch.int64)
    prev = torch.where(pos > 0, torch.roll(b, 1), torch.zeros_like(b))
    sel = mask_of % T == t
    flat = torch.repeat_interleave((pos[sel] % 2).to(torch.uint8), (b - prev)[sel])
    rows = torch.zeros((n, hw), dtype=torch.uint8, device=bounds.device)
    present = per_mask[t::T] > 0
    rows[present] = flat.reshape(int(present.sum()), hw)
    return rows


def vis_overlap_aten(dt_runs, gt_runs, T, H, W):
    """inter int32 [D, G, T] on the runs' device, CPU or GPU: both sides decoded to dense 0 / 1 rows one frame at a time, the counts as
    their product (sums of at most H W ones: exact in float32 below 2^24 pixels, in float64 above)."""
    D, G = _check("vis_overlap_aten", gt_runs, dt_runs, T, H, W)
    T, hw = int(T), int(H) * int(W)
    gt_runs = gt_runs.to(dt_runs.device)
    acc = torch.float32 if hw < 2 ** 24 else torch.float64
    inter = torch.zeros((D, G, T), dtype=torch.int32, device=dt_runs.device)
    for t in range(T):
        d, g = _dense_frame(dt_runs, t, T, hw).to(acc), _dense_frame(gt_runs, t, T, hw).to(acc)
        inter[:, :, t] = (d @ g.T).round().to(torch.int32)
    return inter


def vis_overlap(dt_runs, gt_runs, T, H, W):
    """inter int32 [D, G, T]: the kernel on GPU tensors where it covers the call, else the ATen formulation."""
    return _counts.kernel_else_aten(vis_video_overlap, vis_overlap_aten, dt_runs, gt_runs, T, H, W)
