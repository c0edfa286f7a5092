"""Writes tests/golden/g36_jpeg_encode_pil.npz: the files `PIL.Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s)` of a few small
cases of tests/jpeg_encode_cases.py, from the Pillow this file was made with, so that univs_amd/data/jpeg_encode_rule.py stays pinned to
that encoder whatever Pillow a machine has.

    python tools/gen_golden_jpeg_encode.py
"""
import json
import os
import sys

import numpy as np
import PIL
import PIL.features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpeg_encode_cases as cases  # noqa: E402


def main():
    out = {c.name: np.frombuffer(cases.pillow_file(c.rgb, c.quality, c.sampling), np.uint8) for c in cases.golden_cases()}
    recipe = {"pillow": PIL.__version__, "libjpeg_turbo": PIL.features.version("libjpeg_turbo"), "cases": list(cases.GOLDEN_NAMES)}
    out["recipe"] = np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "g36_jpeg_encode_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__, recipe["libjpeg_turbo"])


if __name__ == "__main__":
    main()
