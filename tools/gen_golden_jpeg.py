"""Writes tests/golden/g35_jpeg_pil.npz: a few small JPEG files of tests/jpeg_cases.py (the files themselves: another libjpeg would encode
other bytes) and the pixels `np.asarray(PIL.Image.open(f).convert("RGB"))` of the Pillow this file was made with, so that
univs_amd/data/jpeg_rule.py stays pinned to that decoder whatever Pillow a machine has.

    python tools/gen_golden_jpeg.py
"""
import json
import os
import sys

import numpy as np
import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import jpeg_cases  # noqa: E402

# one file per sampling and per encoder option, every content kind, low and high quality, odd sizes
NAMES = ("17x31_444", "17x31_420", "40x48_422", "40x48_grey", "75x131_420", "optimize_40x48_420", "restart3_75x131_422", "restartrow_75x131_444",
         "restart3_optimize_17x31_420")


def main():
    out, names = {}, []
    for part in NAMES:
        case = next(c for c in jpeg_cases.covered_cases() if part in c.name)
        names.append(case.name)
        out[case.name + "/file"] = np.frombuffer(case.data, np.uint8)
        out[case.name + "/pixels"] = jpeg_cases.pillow_pixels(case.data)
    recipe = {"pillow": PIL.__version__, "libjpeg_turbo": PIL.features.version("libjpeg_turbo"), "cases": names}
    out["recipe"] = np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "g35_jpeg_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__, recipe["libjpeg_turbo"])


if __name__ == "__main__":
    import PIL.features
    main()
