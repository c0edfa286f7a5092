"""Wrappers of the nineteenth header (include/univs_polygons_hip.h): polygon segmentations to `Runs` (evaluation/vis_counts.py).

  polygons_to_runs              all objects of a call by the kernel (csrc/polygon_runs.hip): one upload, one launch, the compaction of
                                the slots on the device; an object the kernel reports as not covered goes to the host formulation, alone
  polygons_to_runs_status       the same, with the kernel's per-object status
  plan / upload / launch        its three steps before the download, apart (tools/polygon_bench.py times the launch alone)
  polygons_to_runs_else_host    the kernel on a GPU, `polygon_rule.runs_from_polygons_host` on the CPU
  runs_from_segmentations       per mask a polygon list, an RLE dict or None -> one `Runs`
  slice_runs                    a range of masks of a `Runs`

The rule and the host formulation are data/polygon_rule.py.  An object is a list of flat polygons [x0, y0, x1, y1, ...]; None or [] is an
absent mask.  A malformed polygon is a ValueError raised on the host, before anything is uploaded.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, ops
from .data import polygon_rule as rule
from .evaluation._counts import pick_device
from .evaluation.vis_counts import Runs, runs_from_rles

STATUS_TO_HOST = (1, 2, 3, 4)          # include/univs_polygons_hip.h: crossings, points, size, vertices -- rasterised by the host instead
LAST_STATUS = None                      # the kernel's status of the last call, int32 [N] (numpy): what the tests and the bench read


class Plan(NamedTuple):
    """What the host knows of a call before the launch (`plan`)."""
    blob: np.ndarray             # the one upload: xy float64 | slot int64 | poly_start, obj_start, size int32
    offsets: tuple               # the byte offsets of the five tables in it
    slot: np.ndarray             # int64 [N + 1]
    crossings: np.ndarray        # int64 [N]
    points_total: int            # the points the kernel makes
    n_points: int
    P: int
    N: int
    cap_total: int


class OnDevice(NamedTuple):
    tables: torch.Tensor
    bounds: torch.Tensor
    ones: torch.Tensor
    count_status: torch.Tensor   # int32 [2 N]: the counts, then the statuses


def plan(objects, sizes, names=None):
    """The host half: the refusals of a malformed polygon or size, the tables, and both counts the kernel's coverage is stated in --
    known from the scaled vertices --, from which every covered object's slots are sized (an object beyond a cap gets none: the
    kernel says which cap)."""
    xy, poly_start, obj_start, size = rule.pack(objects, sizes, names)
    N, P, n_points = len(objects), poly_start.shape[0] - 1, xy.shape[0] // 2
    crossings, points, verts = rule.crossing_counts(xy, poly_start, obj_start, size)
    covered = (crossings <= rule.MAX_CROSSINGS) & (points <= rule.MAX_POINTS) & (verts <= rule.MAX_VERTS)
    slot = np.concatenate([[0], np.cumsum(np.where(covered & (np.diff(obj_start) > 0), crossings + 1, 0))]).astype(np.int64)
    cap_total = int(slot[-1])
    if n_points >= 2 ** 31 or cap_total >= 2 ** 31:
        raise NotImplementedError(f"polygons_to_runs: {n_points} points / {cap_total} boundaries do not fit 32-bit offsets; split the call")
    parts = (xy.astype(np.float64), slot, poly_start.astype(np.int32), obj_start.astype(np.int32), size.astype(np.int32).reshape(-1))
    blob = np.concatenate([np.ascontiguousarray(p).view(np.uint8) for p in parts] + [np.zeros(8, np.uint8)])      # the 8-byte tables first
    offsets, at = [], 0
    for p in parts:
        offsets.append(at)
        at += p.nbytes
    points_total = int(rule._points_per_object(xy, poly_start, obj_start).sum())
    return Plan(blob, tuple(offsets), slot, crossings, points_total, n_points, P, N, cap_total)


def upload(p, device):
    """The one upload, and the slots, counts and statuses the kernel writes (uninitialised: it writes every count and status)."""
    out = torch.empty(2 * max(p.cap_total, 1), dtype=torch.int32, device=device)
    return OnDevice(torch.from_numpy(p.blob).to(device), out[:max(p.cap_total, 1)], out[max(p.cap_total, 1):],
                    torch.empty(2 * p.N, dtype=torch.int32, device=device))


def launch(p, d):
    """The launch alone, on the tables' device and current stream."""
    base = d.tables.data_ptr()
    xy, slot, poly_start, obj_start, size = (base + o for o in p.offsets)
    ops._call("polygons_to_runs", _lib.load().univs_polygons_to_runs, d.tables, xy, poly_start, obj_start, size, slot, p.n_points, p.P, p.N,
              p.cap_total, ops._ptr(d.bounds), ops._ptr(d.ones), ops._ptr(d.count_status), ops._ptr(d.count_status) + 4 * p.N, uncovered="raise")


def polygons_to_runs_status(objects, sizes, device, names=None):
    """-> (`Runs` on `device`, status int32 [N] as the kernel wrote it).  `device` must be a GPU."""
    name = "polygons_to_runs"
    p = plan(objects, sizes, names)                                                    # the host's refusals come first
    device = torch.device(device)
    if device.type != "cuda":
        raise ops._cpu_refusal(name, f"device {device}")
    N = p.N
    if N == 0:
        z = torch.zeros(0, dtype=torch.int32, device=device)
        return Runs(z, z.clone(), torch.zeros(1, dtype=torch.int32, device=device)), np.zeros(0, np.int32)
    d = upload(p, device)
    launch(p, d)
    slot, bounds, ones, count = p.slot, d.bounds, d.ones, d.count_status[:N]
    cs = d.count_status.cpu().numpy()                                                 # (the one download: 8 bytes per object)
    count_h, status_h = cs[:N].astype(np.int64), cs[N:].copy()
    refused = np.flatnonzero(~np.isin(status_h, (0,) + STATUS_TO_HOST))
    if refused.shape[0]:
        o = int(refused[0])
        raise _lib.UnivsHipError(f"{name}: {names[o] if names else f'object {o}'}: status {int(status_h[o])} for an object the host admitted")
    to_host = np.flatnonzero(status_h != 0)
    host = {int(o): rule.runs_from_polygons_host([objects[o]], [sizes[o]]) for o in to_host}     # one by one; the others are not redone
    per = count_h.copy()
    for o, r in host.items():
        per[o] = r.bounds.numel()
    starts = np.concatenate([[0], np.cumsum(per)])
    if starts[-1] >= 2 ** 31:
        raise NotImplementedError(f"{name}: {int(starts[-1])} boundaries do not fit 32-bit offsets; split the call")
    # the compaction, on the device: element k of object o moves from slot[o] + k to starts[o] + k
    total = int(count_h.sum())
    count_d = count.to(torch.int64)
    obj = torch.repeat_interleave(torch.arange(N, device=device), count_d, output_size=total)
    first = torch.cumsum(count_d, 0) - count_d
    k = torch.arange(total, device=device) - first[obj]
    src = torch.from_numpy(slot[:-1]).to(device)[obj] + k
    if not host:
        fb, fo = bounds[src], ones[src]
    else:
        dst = torch.from_numpy(starts[:-1]).to(device)[obj] + k
        fb = torch.empty(int(starts[-1]), dtype=torch.int32, device=device)
        fo = torch.empty_like(fb)
        fb[dst], fo[dst] = bounds[src], ones[src]
        for o, r in host.items():
            fb[int(starts[o]):int(starts[o + 1])] = r.bounds.to(device)
            fo[int(starts[o]):int(starts[o + 1])] = r.ones.to(device)
    global LAST_STATUS
    LAST_STATUS = status_h
    return Runs(fb, fo, torch.from_numpy(starts.astype(np.int32)).to(device)), status_h


def polygons_to_runs(objects, sizes, device, names=None):
    """`Runs` on the GPU `device` of all objects (per object a list of flat polygons, None or [] for an absent mask; `sizes`: per object
    (h, w), which may differ) by the rule of data/polygon_rule.py.  A CPU device raises, as every wrapper of ops.py does."""
    return polygons_to_runs_status(objects, sizes, device, names)[0]


def polygons_to_runs_else_host(objects, sizes, device=None, names=None):
    """The kernel where `device` is a GPU, else the host formulation on `device`."""
    device = pick_device(device)
    if device.type == "cuda":
        return polygons_to_runs(objects, sizes, device, names)
    return rule.runs_from_polygons_host(objects, sizes, device=device, names=names)


def _merge(parts, n, device):
    """`Runs` of n masks from `parts`, each a `Runs` of n masks on `device`, no mask present in two of them."""
    per = [p.starts.to(torch.int64).diff() for p in parts]
    total = torch.stack(per).sum(0) if per else torch.zeros(n, dtype=torch.int64, device=device)
    starts = torch.cat([total.new_zeros(1), torch.cumsum(total, 0)])
    size = int(sum(p.bounds.numel() for p in parts))
    bounds = torch.empty(size, dtype=torch.int32, device=device)
    ones = torch.empty_like(bounds)
    for p, c in zip(parts, per):
        m = p.bounds.numel()
        obj = torch.repeat_interleave(torch.arange(n, device=device), c, output_size=m)
        dst = starts[obj] + torch.arange(m, device=device) - p.starts.to(torch.int64)[obj]
        bounds[dst], ones[dst] = p.bounds, p.ones
    return Runs(bounds, ones, starts.to(torch.int32))


def runs_from_segmentations(segms, sizes, device=None, names=None):
    """One `Runs` on `device` of `segms`: per mask a list of polygons, an RLE dict ({"size", "counts"}: compressed or uncompressed) or
    None (absent); `sizes`: per mask the (h, w) of its image.  The polygons of all masks are rasterised in ONE
    `polygons_to_runs_else_host` call; the RLE entries go through `runs_from_rles`, one call per image size.  An RLE whose size is
    not its image's is a ValueError that names the mask (`names[i]`)."""
    device = pick_device(device)
    n = len(segms)
    polys, by_size = [None] * n, {}
    for i, s in enumerate(segms):
        if not s:
            continue
        if isinstance(s, dict):
            hw = (int(sizes[i][0]), int(sizes[i][1]))
            if [int(v) for v in s["size"]] != list(hw):
                raise ValueError(f"{names[i] if names else f'mask {i}'}: a mask of size {list(s['size'])} on an image of {list(hw)}")
            by_size.setdefault(hw, []).append(i)
        else:
            polys[i] = s
    parts = []
    if any(p is not None for p in polys) or not by_size:
        parts.append(polygons_to_runs_else_host(polys, sizes, device, names))
    for (h, w), idx in by_size.items():
        rles = [None] * n
        for i in idx:
            rles[i] = segms[i]
        parts.append(runs_from_rles(rles, h, w, device=device))
    return parts[0] if len(parts) == 1 else _merge(parts, n, device)


def slice_runs(runs, a, b, starts_host=None):
    """The masks a .. b of `runs` as a `Runs` of their own.  `starts_host`: the host copy of runs.starts where the caller keeps one
    (a slice then costs no download)."""
    s = starts_host if starts_host is not None else runs.starts.cpu().numpy()
    lo, hi = int(s[a]), int(s[b])
    return Runs(runs.bounds[lo:hi], runs.ones[lo:hi], runs.starts[a:b + 1] - lo)
