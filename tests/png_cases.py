"""The frames of the PNG encoder's tests (test_png_rule_cpu.py, test_png_deflate_gpu.py): pixel bytes [H, W, C] built so that the token
rule of univs_amd/inference/png_rule.py meets every turn it has -- and, for the kernel, as id maps with the look-up table that gives
those bytes.  Most frames are made from an eq pattern (which positions of the filtered row equal the byte d = C places before), so
that run lengths are exact for both distances."""
import functools

import numpy as np

from univs_amd.inference import png_rule

WIDTHS = (1, 2, 3, 258, 259, 260, 261, 517)
R = png_rule.STRIPE_ROWS_MAX                                         # (every width above has R = 16)
HEIGHTS = (1, R - 1, R, R + 1, 2 * R + 1)
SHAPES = ((1, 3), (R - 1, 259), (R + 1, 261), (2 * R + 1, 517))      # where the patterns beyond "zeros" are laid out


def _h(*k):
    """A small deterministic hash of integers."""
    x = 2166136261
    for v in k:
        x = ((x ^ (int(v) & 0xFFFFFFFF)) * 16777619) & 0xFFFFFFFF
    return x


def pixels_from_eq(eq, C, seed=0):
    """eq: bool [H, W C + 1] over the filtered row (position 0 is the filter byte) -> uint8 [H, W, C] whose filtered rows have exactly
    this eq pattern from position d = C on: an eq-true byte copies the byte d before, an eq-false one differs from it."""
    H, n = eq.shape
    rows = np.zeros((H, n), np.uint8)
    for y in range(H):
        for i in range(1, n):
            if i >= C and eq[y, i]:
                rows[y, i] = rows[y, i - C]
            else:
                before = int(rows[y, i - C]) if i >= C else 0
                rows[y, i] = (before + 1 + _h(seed, y, i) % 254) % 256
    return rows[:, 1:].reshape(H, -1, C)


def _eq_cycle(H, W, C, cycle, phase_per_row=1):
    n = W * C + 1
    i = np.arange(n)[None, :] + phase_per_row * np.arange(H)[:, None]
    return np.asarray(cycle, bool)[i % len(cycle)]


def zeros(H, W, C):
    return np.zeros((H, W, C), np.uint8)


def high_literals(H, W, C):
    """Values >= 144 with no byte equal to the one d before: every pixel byte is a 9-bit literal."""
    i = np.arange(W * C)[None, :]
    y = np.arange(H)[:, None]
    return (144 + (i * 37 + y * 11) % 112).astype(np.uint8).reshape(H, W, C)


def period2(H, W, C):
    """Bytes alternate between two values: no match at distance 1 (nor at 3)."""
    i = np.arange(W * C)[None, :] + np.arange(H)[:, None]
    return np.where(i % 2 == 0, 7, 200).astype(np.uint8).reshape(H, W, C)


def runs_2_and_3(H, W, C):
    """eq runs of exactly 2 (two literals) and exactly 3 (the shortest match), alternating."""
    return pixels_from_eq(_eq_cycle(H, W, C, [0, 1, 1, 0, 1, 1, 1]), C, seed=1)


def run_to_row_end(H, W, C):
    """A run that ends at the row's last byte; row y's run has y + 1 bytes (so 1, 2, 3, ... up to the row)."""
    n = W * C + 1
    eq = np.zeros((H, n), bool)
    for y in range(H):
        eq[y, max(C, n - 1 - y):] = True
    return pixels_from_eq(eq, C, seed=2)


def long_runs(H, W, C):
    """Runs of 258 + r bytes, r = 0, 1, 2, 3 by row, each after a few literals (where the row is long enough)."""
    n = W * C + 1
    eq = np.zeros((H, n), bool)
    for y in range(H):
        s = C + 2 + y % 3
        eq[y, s:s + 258 + y % 4] = True
        eq[y, s + 258 + y % 4 + 1:] = True                           # and the rest of the row as one more run
    return pixels_from_eq(eq, C, seed=3)


def blocks7(H, W, C):
    """Random blocks 7 pixels wide and 3 rows high."""
    by, bx = -(-H // 3), -(-W // 7)
    ids = np.array([[_h(4, y, x) % 11 for x in range(bx)] for y in range(by)], np.uint8)
    ids = np.repeat(np.repeat(ids, 3, axis=0), 7, axis=1)[:H, :W]
    return colours(ids, C)


def colours(ids, C):
    if C == 1:
        return ids[..., None].astype(np.uint8)
    k = ids.astype(np.int64)
    return np.stack([k, (k * 7) % 256, (k * 13) % 256], axis=-1).astype(np.uint8)


PATTERNS = (high_literals, period2, runs_2_and_3, run_to_row_end, long_runs, blocks7)


@functools.lru_cache(maxsize=None)
def cases():
    """(name, pixels uint8 [H, W, C])"""
    out = []
    for C in (1, 3):
        for W in WIDTHS:
            for H in HEIGHTS:
                out.append((f"zeros-{H}x{W}x{C}", zeros(H, W, C)))
        for H, W in SHAPES:
            for fn in PATTERNS:
                out.append((f"{fn.__name__}-{H}x{W}x{C}", fn(H, W, C)))
    # the stripe cap: R = 1 with the LDS plan full of 9-bit literals, and R between 1 and 16
    out.append(("high_literals-2x24575x1", high_literals(2, 24575, 1)))
    out.append(("high_literals-3x8191x3", high_literals(3, 8191, 3)))
    out.append(("zeros-2x24575x1", zeros(2, 24575, 1)))
    out.append(("blocks7-5x2000x3", blocks7(5, 2000, 3)))           # row_len 6001: R = 4, two stripes
    out.append(("long_runs-7x3000x1", long_runs(7, 3000, 1)))        # row_len 3001: R = 8
    return out


NOT_COVERED = ("zeros-1x24576x1", zeros(1, png_rule.STRIPE_BYTES, 1))   # a row one byte over the stripe cap


def ids_and_lut(pixels):
    """(ids [H, W] uint8 when the frame has at most 256 colours else int32, lut uint8 [K, C]) with lut[ids] == pixels."""
    H, W, C = pixels.shape
    lut, inv = np.unique(pixels.reshape(-1, C), axis=0, return_inverse=True)
    ids = inv.reshape(H, W)
    return ids.astype(np.uint8 if lut.shape[0] <= 256 else np.int32), np.ascontiguousarray(lut, dtype=np.uint8)
