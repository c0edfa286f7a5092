"""The corpus of the JPEG encoder, generated from seeds: shared by tests/test_jpeg_encode_rule_cpu.py, test_jpeg_encode_gpu.py and
tools/gen_golden_jpeg_encode.py.  The content comes from tests/jpeg_cases.content.

  corpus()         twelve sizes x three contents x three samplings x five qualities, then at 40 x 48 noise at quality 5, 15 and 30 and a
                   checkerboard of two-pixel squares at quality 100, each at the three samplings
  golden_cases()   the few whose Pillow files are recorded in tests/golden/g36_jpeg_encode_pil.npz
  pillow_file(a, quality, sampling)   what the encoder has to give
"""
import functools
import io
from collections import namedtuple

import numpy as np
from PIL import Image

from tests.jpeg_cases import CONTENTS, content

Case = namedtuple("Case", "name rgb quality sampling")

SIZES = ((1, 1), (7, 9), (8, 8), (16, 16), (17, 31), (9, 33), (23, 16), (33, 17), (24, 40), (40, 48), (75, 131), (100, 52))   # (H, W)
SAMPLINGS = ("444", "422", "420")
QUALITIES = (5, 30, 75, 90, 100)
_SUB = {"444": 0, "422": 1, "420": 2}


def checkerboard(H, W, square=2):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((y // square + x // square) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def pillow_file(rgb, quality, sampling):
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, "JPEG", quality=quality, subsampling=_SUB[sampling])
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def corpus():
    out, seed = [], 0
    for H, W in SIZES:
        for kind in CONTENTS:
            a = content(kind, H, W, 3600 + seed)
            a.setflags(write=False)
            seed += 1
            for sampling in SAMPLINGS:
                for quality in QUALITIES:
                    out.append(Case(f"{kind}_{H}x{W}_{sampling}_q{quality}", a, quality, sampling))
    noise = content("noise", 40, 48, 3700)
    board = checkerboard(40, 48)
    for a in (noise, board):
        a.setflags(write=False)
    for sampling in SAMPLINGS:
        for quality in (5, 15, 30):
            out.append(Case(f"morenoise_40x48_{sampling}_q{quality}", noise, quality, sampling))
        out.append(Case(f"checkerboard_40x48_{sampling}_q100", board, 100, sampling))
    return tuple(out)


GOLDEN_NAMES = ("noise_1x1_420_q90", "smooth_7x9_422_q75", "noise_17x31_420_q100", "patches_33x17_444_q30", "noise_40x48_444_q100",
                "morenoise_40x48_420_q15", "checkerboard_40x48_444_q100", "smooth_24x40_420_q90")


def golden_cases():
    by_name = {c.name: c for c in corpus()}
    return tuple(by_name[n] for n in GOLDEN_NAMES)
