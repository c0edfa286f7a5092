"""Writes tests/golden/g32_frames_pil.npz: `PIL.Image.resize(BILINEAR)` of the frames of tests/frames_cases.py (GOLDEN_CASES, every
kind), so that univs_amd/data/resize_rule.py stays pinned to the Pillow this file was made with whatever Pillow a machine has.  The
inputs are closed-form (frames_cases.frames) and are not stored.

    python tools/gen_golden_frames.py
"""
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import frames_cases  # noqa: E402


def main():
    out = {}
    for case in frames_cases.GOLDEN_CASES:
        (T, Hi, Wi), (Ho, Wo) = case
        for kind in frames_cases.KINDS:
            src = frames_cases.frames(kind, T, Hi, Wi)
            out[f"{frames_cases.case_id(case)}/{kind}"] = np.stack([np.asarray(Image.fromarray(f).resize((Wo, Ho), Image.BILINEAR)) for f in src])
    recipe = {"pillow": PIL.__version__, "cases": [frames_cases.case_id(c) for c in frames_cases.GOLDEN_CASES], "kinds": list(frames_cases.KINDS)}
    out["recipe"] = np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "g32_frames_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
