"""Writes tests/golden/g33_prompt_masks_pil.npz: `PIL.Image.resize(NEAREST)` of the masks of tests/prompt_masks_cases.py
(GOLDEN_CASES) with their run-length counts and boxes, so that `nearest_table` / `resize_nearest` of univs_amd/data/resize_rule.py stay
pinned to the Pillow this file was made with whatever Pillow a machine has.

    python tools/gen_golden_prompts.py
"""
import json
import os
import sys

import numpy as np
import PIL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import prompt_masks_cases as pc  # noqa: E402


def main():
    out = {}
    for case in pc.GOLDEN_CASES:
        (kind, H, W), out_hw = case
        m = pc.mask(kind, H, W)
        resized = pc.pillow_resize(m, out_hw)
        name = pc.case_id(case)
        out[f"{name}/counts"] = np.asarray(pc.counts_of(m), np.int32)
        out[f"{name}/mask"] = resized
        out[f"{name}/box"] = pc.any_boxes(resized[None])[0].astype(np.int32)
    recipe = {"pillow": PIL.__version__, "cases": [pc.case_id(c) for c in pc.GOLDEN_CASES]}
    out["recipe"] = np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "g33_prompt_masks_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
