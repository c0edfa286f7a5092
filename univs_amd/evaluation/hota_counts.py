"""The tables of a HOTA evaluation, per video: what TrackEval's `HOTA.eval_sequence` (the reference's univs/evaluation/eval_hota.py:25-117)
accumulates in its frame loops, for every class sequence of the video at once (hota.py).

  hota_video_counts   the HIP kernel (csrc/hota_count.hip) behind `ops._call`: GPU tensors only, None where it does not cover
  hota_counts_aten    the rule in numpy, with one scipy `linear_sum_assignment` per frame as in the reference: the fallback, the
                      yardstick, the CPU path
  hota_counts         the kernel on GPU tensors where it covers the call, else the rule
  lsa_max             the kernel's assignment solver alone, on a batch of small float64 problems

Inputs.  gt_area int32 [G, T] and tr_area int32 [D, T]: the per-frame areas of the video's ground-truth and result tracks, 0 = the id
is absent from the frame.  inter int32 [D, G, T]: the per-frame overlaps as `vis_overlap` returns them.  The class sequences are host
lists: class c owns the ground truths gt_ids[gt_starts[c] : gt_starts[c + 1]] (indices into G) and the tracks
tr_ids[tr_starts[c] : tr_starts[c + 1]] (indices into D).  thresholds: float64 [A], already alpha - eps.

Outputs: `HotaTables`, all on the device of the inputs, per class and packed by the same starts (`HotaTables.of_class` cuts one out):
tp_fn_fp int32 [C, A, 3]; matches int32, [A, g, p] of class c at A sum_{c' < c} g' p'; loca_sum float64 [C, A]; gt_id_count int32 [sum g];
tracker_id_count int32 [sum p]; match_col int32, [T, g] of class c at T gt_starts[c].

The rule.  similarity[g, p] = I / (A_g + A_p - I) in float64 between ids present in the frame.  Pass 1 adds
similarity / (column sum + row sum - similarity), guarded by `> 0 + eps`, to potential_matches_count and counts the frames of every id;
global_alignment_score = pmc / (count_g + count_p - pmc).  Pass 2 assigns, per frame, the present ids so that sum gas similarity is
largest, and tallies per threshold: a matched pair counts where similarity >= alpha - eps; TP, FN, FP; matches[a, g, p] += 1; the frame's
matched similarities are summed from 0 in ascending ground-truth row and that partial sum is added to loca_sum[a].  match_col[t, g] is the
class-local track assigned to ground truth g in frame t if their similarity is above 0, else -1: a pair without overlap passes no
threshold, and which of them an optimal assignment holds is arbitrary, so they are not recorded.

What is pinned.  loca_sum and the integer tables are functions of the per-frame assignment; global_alignment_score only steers it, and the
kernel's need not have numpy's bits (numpy's `sum(1)` is pairwise, the kernel's row sum is serial).  Where a frame's optimum is unique
every optimal solver returns it and the tables are the reference's, loca_sum bit for bit.  Where two assignments of positive pairs reach
the same total both are HOTA-valid and the kernel and scipy may differ; the kernel's rule among equal distances -- an unassigned column
first, then the lowest index -- is this project's choice, not SciPy's.
"""
from typing import NamedTuple

import numpy as np
import torch

from .. import ops
from . import _counts

MAX_IDS = 64          # csrc/hota_count.hip: HO_N, the ids per side of one class sequence (the lanes of a wave)
MAX_THRESHOLDS = 32   # HO_A_MAX
EPS = np.finfo('float').eps


class HotaTables(NamedTuple):
    tp_fn_fp: torch.Tensor
    matches: torch.Tensor
    loca_sum: torch.Tensor
    gt_id_count: torch.Tensor
    tracker_id_count: torch.Tensor
    match_col: torch.Tensor

    def of_class(self, c, gt_starts, tr_starts, T):
        """The tables of class c as numpy arrays: tp_fn_fp [A, 3], matches [A, g, p], loca_sum [A], gt_id_count [g],
        tracker_id_count [p], match_col [T, g]."""
        gs, ps = np.asarray(gt_starts, np.int64), np.asarray(tr_starts, np.int64)
        g, p = int(gs[c + 1] - gs[c]), int(ps[c + 1] - ps[c])
        A = int(self.tp_fn_fp.shape[1])
        mo = A * int((np.diff(gs)[:c] * np.diff(ps)[:c]).sum())
        host = [x.cpu().numpy() for x in self]
        return (host[0][c], host[1][mo:mo + A * g * p].reshape(A, g, p), host[2][c], host[3][gs[c]:gs[c + 1]], host[4][ps[c]:ps[c + 1]],
                host[5][T * gs[c]:T * gs[c + 1]].reshape(T, g))


def _lists(name, G, D, gt_ids, gt_starts, tr_ids, tr_starts):
    """The four host lists as int64 arrays, checked -> (gt_ids, gt_starts, tr_ids, tr_starts, C)."""
    out = []
    for side, ids, starts, n in (("gt", gt_ids, gt_starts, G), ("tracker", tr_ids, tr_starts, D)):
        ids, starts = np.asarray(ids, np.int64).reshape(-1), np.asarray(starts, np.int64).reshape(-1)
        if starts.shape[0] < 2 or starts[0] != 0 or (np.diff(starts) < 0).any() or starts[-1] != ids.shape[0]:
            raise RuntimeError(f"{name}: the {side} starts {starts.tolist()} do not cut {ids.shape[0]} ids into classes")
        if ids.shape[0] and (ids.min() < 0 or ids.max() >= n):
            raise RuntimeError(f"{name}: a {side} id outside 0..{n - 1}")
        out += [ids, starts]
    if out[1].shape[0] != out[3].shape[0]:
        raise RuntimeError(f"{name}: {out[1].shape[0] - 1} gt classes, {out[3].shape[0] - 1} tracker classes")
    return (*out, out[1].shape[0] - 1)


def _check(name, gt_area, tr_area, inter, thresholds):
    """-> (D, G, T, A).  (`gt` first: the order of _counts.admit.)"""
    for what, x, d in (("gt_area", gt_area, 2), ("tr_area", tr_area, 2), ("inter", inter, 3)):
        if x.dtype != torch.int32 or x.dim() != d:
            raise RuntimeError(f"{name}: {what} must be int32 with {d} dimensions, got {x.dtype} {tuple(x.shape)}")
    D, G, T = (int(v) for v in inter.shape)
    if tuple(gt_area.shape) != (G, T) or tuple(tr_area.shape) != (D, T) or D < 1 or G < 1 or T < 1:
        raise RuntimeError(f"{name}: inter {tuple(inter.shape)}, gt_area {tuple(gt_area.shape)}, tr_area {tuple(tr_area.shape)}: "
                           "not [D, G, T], [G, T], [D, T], all non-empty")
    A = int(np.asarray(thresholds).reshape(-1).shape[0])
    if A < 1:
        raise RuntimeError(f"{name}: no thresholds")
    return D, G, T, A


def _empty_tables(C, A, T, gt_starts, tr_starts, device):
    n_g, n_p = int(gt_starts[-1]), int(tr_starts[-1])
    cells = int((np.diff(gt_starts) * np.diff(tr_starts)).sum())
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=device)
    return HotaTables(z((C, A, 3)), z((A * cells,)), z((C, A), torch.float64), z((n_g,)), z((n_p,)),
                      torch.full((T * n_g,), -1, dtype=torch.int32, device=device))


def hota_video_counts(gt_area, tr_area, inter, gt_ids, gt_starts, tr_ids, tr_starts, thresholds):
    """`HotaTables` from csrc/hota_count.hip on the tensors' device and current stream, one launch for all classes; None where the kernel
    does not cover the call (a class with more than MAX_IDS ids on a side, more than MAX_THRESHOLDS thresholds, T > 65535): the caller
    keeps `hota_counts_aten`.  CPU tensors raise, as in every wrapper of ops.py."""
    name = "hota_video_counts"
    D, G, T, A = _counts.admit(name, gt_area, tr_area, _check, inter, thresholds)
    if inter.device != gt_area.device:
        raise RuntimeError(f"{name}: gt_area on {gt_area.device}, inter on {inter.device}")
    gt_ids, gt_starts, tr_ids, tr_starts, C = _lists(name, G, D, gt_ids, gt_starts, tr_ids, tr_starts)
    max_g, max_p = int(np.diff(gt_starts).max()), int(np.diff(tr_starts).max())
    if max_g > MAX_IDS or max_p > MAX_IDS or A > MAX_THRESHOLDS or T > 65535:
        return None
    dev = gt_area.device
    gt_area, tr_area, inter = gt_area.contiguous(), tr_area.contiguous(), inter.contiguous()
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a if a.shape[0] else np.zeros(1, a.dtype))).to(dtype=dt).to(dev)
    lists = [up(a, torch.int32) for a in (gt_ids, gt_starts, tr_ids, tr_starts)]
    thr = up(np.asarray(thresholds, np.float64).reshape(-1), torch.float64)
    out = _empty_tables(C, A, T, gt_starts, tr_starts, dev)
    padded = [x if x.numel() else x.new_zeros(1) for x in out]      # (a side without ids: no NULL pointer)
    r = _counts.launch(name, "univs_hota_counts", gt_area, padded, ops._ptr(inter), ops._ptr(gt_area), ops._ptr(tr_area), D, G, T,
                       ops._ptr(lists[0]), ops._ptr(lists[1]), ops._ptr(lists[2]), ops._ptr(lists[3]), C, max_g, max_p, ops._ptr(thr), A)
    return None if r is None else out


def sequence_counts(sim, present_g, present_p, thresholds):
    """The rule on one class sequence.  sim: float64 [T, g, p], the similarities (read only where both ids are present); present_g
    bool [T, g], present_p bool [T, p] -> (tp_fn_fp [A, 3], matches [A, g, p], loca_sum [A], gt_id_count [g], tracker_id_count [p],
    match_col [T, g]).  The statements are eval_hota.py:47-101's, on the frame's present ids."""
    from scipy.optimize import linear_sum_assignment
    T, g, p = sim.shape
    A = len(thresholds)
    gt_ids = [np.flatnonzero(present_g[t]) for t in range(T)]
    tracker_ids = [np.flatnonzero(present_p[t]) for t in range(T)]
    similarity_scores = [sim[t][np.ix_(gt_ids[t], tracker_ids[t])] for t in range(T)]
    potential_matches_count = np.zeros((g, p))
    gt_id_count = np.zeros((g, 1))
    tracker_id_count = np.zeros((1, p))
    for t, (gt_ids_t, tracker_ids_t) in enumerate(zip(gt_ids, tracker_ids)):
        similarity = similarity_scores[t]
        sim_iou_denom = similarity.sum(0)[np.newaxis, :] + similarity.sum(1)[:, np.newaxis] - similarity
        sim_iou = np.zeros_like(similarity)
        sim_iou_mask = sim_iou_denom > 0 + EPS
        sim_iou[sim_iou_mask] = similarity[sim_iou_mask] / sim_iou_denom[sim_iou_mask]
        potential_matches_count[gt_ids_t[:, np.newaxis], tracker_ids_t[np.newaxis, :]] += sim_iou
        gt_id_count[gt_ids_t] += 1
        tracker_id_count[0, tracker_ids_t] += 1
    with np.errstate(divide="ignore", invalid="ignore"):              # (0 / 0 where an id never occurs: never indexed below)
        global_alignment_score = potential_matches_count / (gt_id_count + tracker_id_count - potential_matches_count)
    tp_fn_fp = np.zeros((A, 3), np.int32)
    matches = np.zeros((A, g, p), np.int32)
    loca_sum = np.zeros(A, np.float64)
    match_col = np.full((T, g), -1, np.int32)
    for t, (gt_ids_t, tracker_ids_t) in enumerate(zip(gt_ids, tracker_ids)):
        if len(gt_ids_t) == 0:
            tp_fn_fp[:, 2] += len(tracker_ids_t)
            continue
        if len(tracker_ids_t) == 0:
            tp_fn_fp[:, 1] += len(gt_ids_t)
            continue
        similarity = similarity_scores[t]
        score_mat = global_alignment_score[gt_ids_t[:, np.newaxis], tracker_ids_t[np.newaxis, :]] * similarity
        match_rows, match_cols = linear_sum_assignment(-score_mat)
        overlap = similarity[match_rows, match_cols] > 0
        match_col[t, gt_ids_t[match_rows[overlap]]] = tracker_ids_t[match_cols[overlap]]
        for a, alpha_eps in enumerate(thresholds):
            actually_matched_mask = similarity[match_rows, match_cols] >= alpha_eps
            alpha_match_rows = match_rows[actually_matched_mask]
            alpha_match_cols = match_cols[actually_matched_mask]
            num_matches = len(alpha_match_rows)
            tp_fn_fp[a] += (num_matches, len(gt_ids_t) - num_matches, len(tracker_ids_t) - num_matches)
            if num_matches > 0:
                loca_sum[a] += sum(similarity[alpha_match_rows, alpha_match_cols])
                matches[a][gt_ids_t[alpha_match_rows], tracker_ids_t[alpha_match_cols]] += 1
    return tp_fn_fp, matches, loca_sum, gt_id_count[:, 0].astype(np.int32), tracker_id_count[0].astype(np.int32), match_col


def similarities(gt_area, tr_area, inter):
    """float64 [T, g, p] from int [g, T], [p, T], [p, g, T] numpy arrays: I / (A_g + A_p - I) where both ids are present, 0 elsewhere."""
    i = inter.transpose(2, 1, 0).astype(np.int64)
    u = gt_area.T.astype(np.int64)[:, :, None] + tr_area.T.astype(np.int64)[:, None, :] - i
    both = (gt_area.T > 0)[:, :, None] & (tr_area.T > 0)[:, None, :]
    return np.where(both, i.astype(np.float64) / np.where(both, u, 1).astype(np.float64), 0.0)


def hota_counts_aten(gt_area, tr_area, inter, gt_ids, gt_starts, tr_ids, tr_starts, thresholds):
    """`HotaTables` on the tensors' device, CPU or GPU, by the rule in numpy on the host, class by class."""
    name = "hota_counts_aten"
    D, G, T, A = _check(name, gt_area, tr_area, inter, thresholds)
    gt_ids, gt_starts, tr_ids, tr_starts, C = _lists(name, G, D, gt_ids, gt_starts, tr_ids, tr_starts)
    thresholds = np.asarray(thresholds, np.float64).reshape(-1)
    ga, ta, it = gt_area.cpu().numpy(), tr_area.cpu().numpy(), inter.cpu().numpy()
    out = [x.cpu().numpy().copy() for x in _empty_tables(C, A, T, gt_starts, tr_starts, "cpu")]
    mo = 0
    for c in range(C):
        gi, pi = gt_ids[gt_starts[c]:gt_starts[c + 1]], tr_ids[tr_starts[c]:tr_starts[c + 1]]
        g, p = len(gi), len(pi)
        a_g, a_p = ga[gi], ta[pi]
        tables = sequence_counts(similarities(a_g, a_p, it[np.ix_(pi, gi)]), a_g.T > 0, a_p.T > 0, thresholds)
        out[0][c], out[2][c] = tables[0], tables[2]
        out[1][mo:mo + A * g * p] = tables[1].reshape(-1)
        out[3][gt_starts[c]:gt_starts[c + 1]], out[4][tr_starts[c]:tr_starts[c + 1]] = tables[3], tables[4]
        out[5][T * gt_starts[c]:T * gt_starts[c + 1]] = tables[5].reshape(-1)
        mo += A * g * p
    return HotaTables(*(torch.from_numpy(x).to(gt_area.device) for x in out))


def hota_counts(gt_area, tr_area, inter, gt_ids, gt_starts, tr_ids, tr_starts, thresholds):
    """`HotaTables`: the kernel on GPU tensors where it covers the call, else the rule."""
    return _counts.kernel_else_aten(hota_video_counts, hota_counts_aten, gt_area, tr_area, inter, gt_ids, gt_starts, tr_ids, tr_starts, thresholds)


def lsa_max(score, rows, cols):
    """The kernel's solver alone.  score: float64 [B, 64, 64] on the GPU; problem b is its top-left rows[b] x cols[b] corner and is
    maximised.  rows, cols: int32 [B] on the same device, each in 1..64.  -> int32 [B, 64]: the column of every row r < rows[b], -1 for
    the rows left over when rows[b] > cols[b] and for r >= rows[b]."""
    name = "lsa_max"
    for x in (score, rows, cols):
        if not x.is_cuda:
            raise ops._cpu_refusal(name, f"tensor on {x.device}")
    B = int(score.shape[0])
    if score.dtype != torch.float64 or tuple(score.shape) != (B, MAX_IDS, MAX_IDS) or not score.is_contiguous():
        raise RuntimeError(f"{name}: score must be contiguous float64 [B, {MAX_IDS}, {MAX_IDS}], got {score.dtype} {tuple(score.shape)}")
    for x in (rows, cols):
        if x.dtype != torch.int32 or tuple(x.shape) != (B,) or x.device != score.device or not x.is_contiguous():
            raise RuntimeError(f"{name}: rows and cols must be int32 [B] on the device of score")
    out = torch.full((B, MAX_IDS), -1, dtype=torch.int32, device=score.device)
    if B:
        _counts.launch(name, "univs_lsa_max_f64", score, (out,), ops._ptr(score), ops._ptr(rows), ops._ptr(cols), B)
    return out
