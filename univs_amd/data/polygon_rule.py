"""Polygon segmentations (COCO's instance ground truth) to run-length codes: the rule, stated once.

This is this project's restatement of the COCO API's published `rleFrPoly` / `frPyObjects` + `merge`; pycocotools is not available
where this project is built, so nothing here is compared with its code.  What pins the rule are cases derivable by hand (integer
rectangles) and three anchors (tests/test_polygon_rule_cpu.py).

  polygon_counts(xy, h, w)             the literal serial rule for ONE polygon -> its run lengths (column-major, the first run background)
  polygon_boundaries_parity(xy, h, w)  the same polygon through the parity form the kernel uses -> its cumulative boundaries
  object_runs(polygons, h, w)          ONE object (the union of its polygons) -> its canonical cumulative boundaries, ending in h w
  check_polygon(xy, what)              the four refusals: odd length, fewer than 6 numbers, a non-finite number, |coordinate| > 2^24
  runs_from_polygons_host(objects, sizes)   numpy over all points of all polygons -> `Runs`: the CPU path, the fallback, the yardstick
  pack(objects, sizes)                 the checked tables of a call: xy, poly_start, obj_start, size
  crossing_counts(*pack(...))          per object, from the scaled vertices alone: its crossings, the points and the vertices of its longest polygon

The rule.  A polygon is a flat list [x0, y0, x1, y1, ...] of k >= 3 points in float64; the image is h x w.  float64, unfused; int(.)
is C's conversion (toward zero).
 1. X[j] = int(5 x_j + 0.5), Y[j] = int(5 y_j + 0.5); X[k] = X[0], Y[k] = Y[0].
 2. Edge j has max(dx, dy) + 1 points from its start to its end, dx = |X[j+1] - X[j]|, dy = |Y[j+1] - Y[j]|.  Where dx >= dy: (xs, ys) is
    the end with the smaller x (the start when dx = 0), s = (ye - ys) / dx (0 when dx = 0), the point at offset t is
    (xs + t, int(ys + s t + 0.5)).  Otherwise (xs, ys) is the end with the smaller y, s = (xe - xs) / dy, the point at offset t is
    (int(xs + s t + 0.5), ys + t).  t runs downward when the ends were exchanged.  (u, v) is the concatenation over the edges.
 3. For j = 1 .. m - 1 with u[j] != u[j-1]: xd = (side + 0.5) / 5 - 0.5 with side = u[j] if u[j] < u[j-1] else u[j] - 1; skipped unless
    xd is an integer in [0, w - 1]; yd = (min(v[j], v[j-1]) + 0.5) / 5 - 0.5 clamped to [0, h], then ceil; the position is xd h + yd.
 4. Append h w, sort, take differences; a zero difference is dropped together with the count after it, which is added to the one
    before.  Equivalently (checked in the tests): the boundaries are the ascending positions < h w that occur an odd number of times,
    then h w.  Odd runs are foreground; the first boundary may be 0.
 5. An object is the union of its polygons' masks.
"""
import math

import numpy as np
import torch

COORD_LIMIT = float(2 ** 24)
MAX_CROSSINGS = 16384          # csrc/polygon_core.h: PG_MAX_KEYS
MAX_POINTS = 1 << 22           # PG_MAX_POINTS
MAX_VERTS = 4096               # PG_MAX_VERTS


def check_polygon(xy, what="the polygon"):
    """The flat coordinate list as float64, or the ValueError that names `what`."""
    try:
        a = np.asarray(xy, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: a polygon is a flat list of numbers") from None
    if a.shape[0] % 2:
        raise ValueError(f"{what}: a polygon of {a.shape[0]} numbers (an odd count)")
    if a.shape[0] < 6:
        raise ValueError(f"{what}: a polygon of {a.shape[0]} numbers (fewer than 3 points)")
    if not np.isfinite(a).all():
        raise ValueError(f"{what}: a polygon with a non-finite coordinate")
    if (np.abs(a) > COORD_LIMIT).any():
        raise ValueError(f"{what}: a polygon with a coordinate beyond 2^24")
    return a


# ---- the literal rule -----------------------------------------------------------------------------------------------------------------------
def _points(xy):
    """Steps 1 and 2 -> (u, v), lists of ints."""
    k = len(xy) // 2
    X = [int(5.0 * float(xy[2 * j]) + 0.5) for j in range(k)]
    Y = [int(5.0 * float(xy[2 * j + 1]) + 0.5) for j in range(k)]
    X.append(X[0])
    Y.append(Y[0])
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ye - ys)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = 0.0 if dx == 0 else float(ye - ys) / float(dx)
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                v.append(int(float(ys) + s * float(t) + 0.5))
        else:
            s = float(xe - xs) / float(dy)
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(float(xs) + s * float(t) + 0.5))
    return u, v


def _positions(xy, h, w):
    """Steps 1 to 3 -> the recorded positions, in the order met."""
    u, v = _points(xy)
    out = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + 0.5) / 5.0 - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + 0.5) / 5.0 - 0.5
        yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
        yd = math.ceil(yd)
        out.append(int(xd * h + yd))
    return out


def polygon_counts(xy, h, w):
    """The run lengths of one polygon on an h x w image by the literal rule (steps 1 to 4)."""
    xy = check_polygon(xy)
    a = sorted(_positions(xy, int(h), int(w)) + [int(h) * int(w)])
    p, diffs = 0, []
    for t in a:
        diffs.append(t - p)
        p = t
    b, j = [diffs[0]], 1
    while j < len(diffs):
        if diffs[j] > 0:
            b.append(diffs[j])
            j += 1
        else:
            j += 1
            if j < len(diffs):
                b[-1] += diffs[j]
                j += 1
    return b


def polygon_boundaries_parity(xy, h, w):
    """One polygon through steps 1 to 3 in their integer form (the column exists where the smaller side is 2 mod 5, the row is
    ceil((vmin - 2) / 5) clamped) and the parity form of step 4 -> its cumulative boundaries, ending in h w."""
    xy = check_polygon(xy)
    h, w = int(h), int(w)
    u, v = _points(xy)
    seen = {}
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        side = u[j] if u[j] < u[j - 1] else u[j] - 1
        if side % 5 != 2:
            continue
        col = (side - 2) // 5
        if col < 0 or col > w - 1:
            continue
        row = min(max(-((2 - min(v[j], v[j - 1])) // 5), 0), h)           # ceil((vmin - 2) / 5) = -floor((2 - vmin) / 5)
        pos = col * h + row
        seen[pos] = seen.get(pos, 0) + 1
    return sorted(p for p, c in seen.items() if c % 2 and p < h * w) + [h * w]


def dense_from_counts(counts, h, w):
    """bool [h, w] of column-major run lengths (the first run is background)."""
    flat = np.repeat(np.arange(len(counts)) % 2 == 1, np.asarray(counts, dtype=np.int64))
    return flat.reshape(int(w), int(h)).T


def boundaries_from_dense(mask):
    """The canonical cumulative column-major boundaries of a bool [h, w]: the first one 0 where pixel 0 is set, the last one h w."""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    change = np.flatnonzero(np.concatenate([[flat[0]], flat[1:] != flat[:-1]])) if flat.shape[0] else np.zeros(0, np.int64)
    return [int(c) for c in change] + [int(flat.shape[0])]


def object_runs(polygons, h, w):
    """One object: the dense OR of its polygons' masks by the literal rule -> the cumulative boundaries of the union ([] without polygons)."""
    if len(polygons) == 0:
        return []
    mask = np.zeros((int(h), int(w)), dtype=bool)
    for xy in polygons:
        mask |= dense_from_counts(polygon_counts(xy, h, w), h, w)
    return boundaries_from_dense(mask)


# ---- numpy over all points of all polygons ------------------------------------------------------------------------------------------------
def _trunc(a):
    return np.trunc(a).astype(np.int64)


def pack(objects, sizes, names=None):
    """`objects`: per object a list of flat polygons; `sizes`: per object (h, w) -> (xy float64 [2 n], poly_start int64 [P + 1] in points,
    obj_start int64 [N + 1] in polygons, size int64 [N, 2]) after `check_polygon` on every polygon (`names[o]` names object o in the
    error) and the check of the sizes."""
    n = len(objects)
    size = np.asarray(sizes, dtype=np.int64).reshape(n, 2) if n else np.zeros((0, 2), np.int64)
    if n and ((size < 1).any() or (size[:, 0] * size[:, 1] >= 2 ** 31).any()):
        bad = int(np.flatnonzero((size < 1).any(axis=1) | (size[:, 0] * size[:, 1] >= 2 ** 31))[0])
        raise ValueError(f"{names[bad] if names else f'object {bad}'}: an image of {size[bad, 0]} x {size[bad, 1]}")
    polys, per_obj = [], []
    for o, obj in enumerate(objects):
        what = names[o] if names else f"object {o}"
        if obj is None:
            obj = ()
        if len(obj) and not isinstance(obj[0], (list, tuple, np.ndarray)):
            raise ValueError(f"{what}: an object is a list of polygons, each a flat list of numbers")
        for i, xy in enumerate(obj):
            polys.append(check_polygon(xy, f"{what}, polygon {i}"))
        per_obj.append(len(obj))
    xy = np.concatenate(polys) if polys else np.zeros(0, np.float64)
    poly_start = np.concatenate([[0], np.cumsum([p.shape[0] // 2 for p in polys], dtype=np.int64)]).astype(np.int64)
    obj_start = np.concatenate([[0], np.cumsum(per_obj, dtype=np.int64)]).astype(np.int64)
    return xy, poly_start, obj_start, size


def _edges(xy, poly_start):
    """Step 1 and the per-edge quantities of step 2, over all edges of all polygons (edge j of a polygon starts at its point j)."""
    X, Y = _trunc(5.0 * xy[0::2] + 0.5), _trunc(5.0 * xy[1::2] + 0.5)
    k = np.diff(poly_start)
    poly = np.repeat(np.arange(k.shape[0]), k)
    nxt = np.arange(X.shape[0]) + 1
    last = poly_start[1:] - 1
    nxt[last[k > 0]] = poly_start[:-1][k > 0]
    xs, ys, xe, ye = X, Y, X[nxt], Y[nxt]
    dx, dy = np.abs(xe - xs), np.abs(ye - ys)
    return poly, xs, ys, xe, ye, dx, dy


def crossing_counts(xy, poly_start, obj_start, size):
    """From the scaled vertices alone, per object: (its crossings -- the columns c in [0, w - 1] whose centre line 5 c + 2 every edge
    passes, summed over its edges --, the points of its longest polygon, the vertices of its longest polygon), int64 [N] each."""
    N = obj_start.shape[0] - 1
    if xy.shape[0] == 0:
        z = np.zeros(N, np.int64)
        return z, z.copy(), z.copy()
    poly, xs, ys, xe, ye, dx, dy = _edges(xy, poly_start)
    obj_of_poly = np.repeat(np.arange(N), np.diff(obj_start))
    w = size[obj_of_poly, 1][poly]
    # the u of an edge's ends as emitted: exact where dx >= dy, int(x + 0.5) otherwise (one more below zero, where no column is)
    steep = dx < dy
    ua = np.where(steep, _trunc(xs + 0.5), xs)
    ub = np.where(steep, _trunc(xe + 0.5), xe)
    lo, hi = np.minimum(ua, ub), np.maximum(ua, ub) - 1                 # the smaller sides met: lo .. hi
    c_lo = np.maximum(-((2 - lo) // 5), 0)                              # ceil((lo - 2) / 5)
    c_hi = np.minimum((hi - 2) // 5, w - 1)
    per_edge = np.maximum(c_hi - c_lo + 1, 0)
    P = poly_start.shape[0] - 1
    cross_poly = np.bincount(poly, weights=per_edge, minlength=P).astype(np.int64)
    points_poly = np.bincount(poly, weights=np.maximum(dx, dy) + 1, minlength=P).astype(np.int64)
    crossings = np.bincount(obj_of_poly, weights=cross_poly, minlength=N).astype(np.int64)
    points = np.zeros(N, np.int64)
    verts = np.zeros(N, np.int64)
    np.maximum.at(points, obj_of_poly, points_poly)
    np.maximum.at(verts, obj_of_poly, np.diff(poly_start))
    return crossings, points, verts


def _points_per_object(xy, poly_start, obj_start):
    """int64 [N]: the points of every object's polygons together."""
    N = obj_start.shape[0] - 1
    if xy.shape[0] == 0:
        return np.zeros(N, np.int64)
    poly, _, _, _, _, dx, dy = _edges(xy, poly_start)
    obj_of_poly = np.repeat(np.arange(N), np.diff(obj_start))
    return np.bincount(obj_of_poly[poly], weights=np.maximum(dx, dy) + 1, minlength=N).astype(np.int64)


def _batch_boundaries(xy, poly_start, obj_start, size):
    """The cumulative boundaries of the objects of one batch -> (bounds int64 back to back, per-object counts int64 [N])."""
    N = obj_start.shape[0] - 1
    present = np.diff(obj_start) > 0
    hw_obj = size[:, 0] * size[:, 1]
    if xy.shape[0] == 0:
        return hw_obj[present], present.astype(np.int64)
    poly, xs, ys, xe, ye, dx, dy = _edges(xy, poly_start)
    flat = dx >= dy
    flip = np.where(flat, xs > xe, ys > ye)
    xs, xe = np.where(flip, xe, xs), np.where(flip, xs, xe)
    ys, ye = np.where(flip, ye, ys), np.where(flip, ys, ye)
    n = np.maximum(dx, dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(flat, np.where(dx == 0, 0.0, (ye - ys).astype(np.float64) / dx.astype(np.float64)),
                     (xe - xs).astype(np.float64) / dy.astype(np.float64))
    # the points: edge-major, d from the edge's original start
    cnt = n + 1
    edge = np.repeat(np.arange(cnt.shape[0]), cnt)
    d = np.arange(edge.shape[0]) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    t = np.where(flip[edge], n[edge] - d, d)
    fe = flat[edge]
    tf = t.astype(np.float64)
    along = _trunc(np.where(fe, ys[edge], xs[edge]).astype(np.float64) + s[edge] * tf + 0.5)
    u = np.where(fe, t + xs[edge], along)
    v = np.where(fe, along, t + ys[edge])
    pp = poly[edge]                                                       # the polygon of every point
    # step 3 in integers, on successive points of one polygon
    ok = (pp[1:] == pp[:-1]) & (u[1:] != u[:-1])
    side = np.where(u[1:] < u[:-1], u[1:], u[1:] - 1)
    obj_of_poly = np.repeat(np.arange(N), np.diff(obj_start))
    po = obj_of_poly[pp[1:]]
    h, w = size[po, 0], size[po, 1]
    col = (side - 2) // 5
    ok &= (side % 5 == 2) & (col >= 0) & (col <= w - 1)
    row = np.clip(-((2 - np.minimum(v[1:], v[:-1])) // 5), 0, h)
    pos = (col * h + row)[ok]
    pid = pp[1:][ok]
    keep = pos < (h * w)[ok]
    pos, pid = pos[keep], pid[keep]
    # step 4 by parity, per polygon
    key = pid * (2 ** 31) + pos
    uniq, c = np.unique(key, return_counts=True)
    uniq = uniq[c % 2 == 1]
    pid, pos = uniq >> 31, uniq & (2 ** 31 - 1)
    # step 5: a polygon's boundaries alternately open (+1) and close (-1) coverage; per object, a boundary where it passes 0 <-> positive
    first = np.concatenate([[True], pid[1:] != pid[:-1]]) if pid.shape[0] else np.zeros(0, bool)
    start = np.flatnonzero(first)
    rank = np.arange(pid.shape[0]) - np.repeat(start, np.diff(np.concatenate([start, [pid.shape[0]]])))
    delta = np.where(rank % 2 == 0, 1, -1)
    oid = obj_of_poly[pid]
    okey = oid * (2 ** 31) + pos
    order = np.argsort(okey, kind="stable")
    okey, delta = okey[order], delta[order]
    last = np.concatenate([okey[1:] != okey[:-1], [True]]) if okey.shape[0] else np.zeros(0, bool)
    cover = np.cumsum(delta)[last]                                        # (every object's deltas sum to 0 or 1 run open to h w ...)
    okey = okey[last]
    oid, pos = okey >> 31, okey & (2 ** 31 - 1)
    # coverage restarts per object: subtract what the objects before left open
    net = np.bincount(oid, weights=np.diff(np.concatenate([[0], cover])), minlength=N).astype(np.int64) if oid.shape[0] else np.zeros(N, np.int64)
    base = np.cumsum(net) - net
    after = cover - base[oid]
    firsto = np.concatenate([[True], oid[1:] != oid[:-1]]) if oid.shape[0] else np.zeros(0, bool)
    before = np.where(firsto, 0, np.concatenate([[0], after[:-1]]))
    b = (before > 0) != (after > 0)
    oid, pos = oid[b], pos[b]
    per_obj = np.bincount(oid, minlength=N).astype(np.int64) + present
    # every present object's list ends in h w
    out = np.empty(int(per_obj.sum()), np.int64)
    ends = np.cumsum(per_obj) - 1
    is_end = np.zeros(out.shape[0], bool)
    is_end[ends[present]] = True
    out[is_end] = hw_obj[present]
    out[~is_end] = pos
    return out, per_obj


def runs_from_boundaries(bounds, per_obj, device=None):
    """int64 boundaries back to back and their per-object counts -> `Runs` (ones: the foreground pixels before every boundary)."""
    from ..evaluation.vis_counts import Runs, _segment_cumsum
    starts = np.concatenate([[0], np.cumsum(per_obj)]).astype(np.int64)
    if starts[-1] >= 2 ** 31:
        raise ValueError(f"{int(starts[-1])} run boundaries do not fit 32-bit offsets")
    sid = np.repeat(np.arange(per_obj.shape[0]), per_obj)
    k = np.arange(bounds.shape[0]) - np.repeat(starts[:-1], per_obj)
    prev = np.where(k > 0, np.concatenate([[0], bounds[:-1]]), 0)
    ones = _segment_cumsum(np.where(k % 2 == 1, bounds - prev, 0), sid)
    return Runs(*(torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(device or "cpu") for a in (bounds, ones, starts)))


def runs_from_polygons_host(objects, sizes, device=None, names=None, batch_points=1 << 22):
    """`Runs` of all objects (per object a list of flat polygons, None or [] for an absent one; `sizes`: per object (h, w)) by the rule,
    in numpy over all points of all polygons of a batch of objects (`batch_points`: about as many points per batch)."""
    xy, poly_start, obj_start, size = pack(objects, sizes, names)
    N = len(objects)
    if N == 0:
        return runs_from_boundaries(np.zeros(0, np.int64), np.zeros(0, np.int64), device)
    # batches of whole objects by their point counts (known from the scaled vertices)
    pts_obj = _points_per_object(xy, poly_start, obj_start)
    cuts, run = [0], 0
    for o in range(N):
        if run and run + pts_obj[o] > batch_points:
            cuts.append(o)
            run = 0
        run += pts_obj[o]
    cuts.append(N)
    bounds, counts = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        p0, p1 = int(obj_start[a]), int(obj_start[b])
        q0, q1 = int(poly_start[p0]), int(poly_start[p1])
        bb, cc = _batch_boundaries(xy[2 * q0:2 * q1], poly_start[p0:p1 + 1] - q0, obj_start[a:b + 1] - p0, size[a:b])
        bounds.append(bb)
        counts.append(cc)
    return runs_from_boundaries(np.concatenate(bounds), np.concatenate(counts), device)
