"""The test-time resize of a frame as integers: the size rule of detectron2's `ResizeShortestEdge` and the 8-bit bilinear of
`PIL.Image.resize`, which detectron2's `ResizeTransform` calls for uint8 images.  Pure numpy, no torch: this is the statement that
csrc/frame_resize.hip is held to (tests/test_frames_rule_cpu.py pins it to Pillow itself and to tests/golden/g32_frames_pil.npz).

Pillow's 8-bit resize is two passes, horizontal then vertical, each a weighted sum with 22-bit integer coefficients, rounded and
clamped to uint8 -- the image is uint8 between the passes, so the intermediate rounding is part of the answer.  A pass whose axis
keeps its size is skipped.  The coefficient tables are computed in float64 exactly as Pillow's `precompute_coeffs` /
`normalize_coeffs_8bpc` do (its bilinear filter has support 1).  Pillow multiplies by the reciprocal of the filter scale where the
formula divides by the scale; this file multiplies too (no integer coefficient differed between the two for any pair of sizes below
400, so the choice is caution, not a known difference).

`shortest_edge_size` restates detectron2 (absent here), so it is not pinned to the reference's code, only to worked examples.

Masks are resized with `PIL.Image.resize(..., NEAREST)` (detectron2's `ResizeTransform.apply_segmentation`).  Per axis Pillow walks
a float64 source coordinate: a = n_in / n_out, xo = a / 2, and for every output index in turn src = int(xo), xo += a.  The sum is
ACCUMULATED; the closed form floor((i + 0.5) a) is a different table (first at 2 -> 7) and not Pillow's.  `nearest_table` is that
loop, `resize_nearest` the gather; csrc/mask_prompt_resize.hip takes the tables as arguments (tests/test_prompt_masks_rule_cpu.py pins
them to Pillow itself and to tests/golden/g33_prompt_masks_pil.npz).
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2                                          # Pillow's: coefficients are scaled by 2^22
KSIZE_MAX = 9                                                        # what csrc/frame_resize.hip covers per axis: a down-scale up to 4


def shortest_edge_size(h, w, short, max_size):
    """(newh, neww) of detectron2's `ResizeShortestEdge.get_output_shape`: the short side becomes `short`, the other keeps the ratio;
    if the longer then exceeds `max_size` both are scaled down to it; each is rounded half up."""
    h, w, short, max_size = int(h), int(w), int(short), int(max_size)
    scale = short * 1.0 / min(h, w)
    if h < w:
        newh, neww = float(short), scale * w
    else:
        newh, neww = scale * h, float(short)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def axis_ksize(n_in, n_out):
    """Slots per output index of `resize_tables(n_in, n_out)`."""
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def resize_tables(n_in, n_out):
    """(first[n_out] int32, count[n_out] int32, coef[n_out, ksize] int32) of one axis: output i is
    clamp((2^21 + sum_{x < count[i]} coef[i, x] * in[first[i] + x]) >> 22).  Unused slots are 0."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"resize_tables: n_in={n_in} n_out={n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs                                                     # (the bilinear filter's support is 1)
    ss = 1.0 / fs
    ksize = axis_ksize(n_in, n_out)
    first = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        n = hi - lo
        ws, total = [], 0.0
        for x in range(n):
            w = max(0.0, 1.0 - abs((x + lo - center + 0.5) * ss))
            ws.append(w)
            total += w
        first[i], count[i] = lo, n
        for x, w in enumerate(ws):
            if total != 0.0:
                w = w / total
            coef[i, x] = int(0.5 + w * (1 << PRECISION_BITS))
    return first, count, coef


def _pass(a, n_out, axis):
    """One pass over `axis` of the uint8 array `a`."""
    first, count, coef = resize_tables(a.shape[axis], n_out)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + a.shape[1:], np.int64)
    for i in range(n_out):
        taps = a[first[i]:first[i] + count[i]]
        k = coef[i, :count[i]].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        out[i] = ((1 << (PRECISION_BITS - 1)) + (taps * k).sum(0)) >> PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize_u8_reference(a, newh, neww):
    """uint8 [H, W] or [H, W, C] -> uint8 [newh, neww(, C)]: `PIL.Image.resize((neww, newh), BILINEAR)` bit for bit."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError(f"resize_u8_reference: uint8 [H, W(, C)], got {a.dtype} {a.shape}")
    if int(neww) != a.shape[1]:
        a = _pass(a, int(neww), 1)
    if int(newh) != a.shape[0]:
        a = _pass(a, int(newh), 0)
    return np.ascontiguousarray(a)


def nearest_table(n_in, n_out):
    """int32 [n_out]: the source index of every output index of one axis under Pillow's NEAREST, by Pillow's own running sum in
    float64 (not the closed form: see the module's docstring)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"nearest_table: n_in={n_in} n_out={n_out}")
    a = n_in / n_out
    xo = a * 0.5
    table = np.empty(n_out, np.int32)
    for i in range(n_out):
        table[i] = int(xo)
        xo += a
    return np.minimum(table, n_in - 1)                                # (never taken for a table Pillow accepts; a bound all the same)


def resize_nearest(mask, newh, neww):
    """[H, W(, C)] -> [newh, neww(, C)] of the same dtype: `PIL.Image.resize((neww, newh), NEAREST)` element for element."""
    mask = np.asarray(mask)
    if mask.ndim not in (2, 3):
        raise ValueError(f"resize_nearest: [H, W(, C)], got {mask.shape}")
    ty, tx = nearest_table(mask.shape[0], newh), nearest_table(mask.shape[1], neww)
    return np.ascontiguousarray(mask[ty][:, tx])
