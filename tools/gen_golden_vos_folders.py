"""Writes tests/golden/g37_vos_folders_pil.npz: for the id maps of tests/idmap_cases.py (GOLDEN_CASES), per value that occurs (and one that
does not) `PIL.Image.resize(NEAREST)` of that value's own plane, with the boxes -- and the resize of the id map itself in palette mode --
so that univs_amd/data/idmap_rule.py stays pinned to the Pillow this file was made with whatever Pillow a machine has.  Pillow only: the
reference is not read.

    python tools/gen_golden_vos_folders.py
"""
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import idmap_cases as ic  # noqa: E402
from tests import prompt_masks_cases as pc  # noqa: E402

VALUES = (0, 1, 2, 255, 9)                                           # (9 never occurs)


def golden_idmap(H, W):
    return ic.idmap("noise" if H * W < 100 else "regions", H, W, (0, 1, 2, 255))


def main():
    out = {}
    for case in ic.GOLDEN_CASES:
        (H, W), out_hw = case
        m = golden_idmap(H, W)
        name = ic.case_id(case)
        planes = np.stack([pc.pillow_resize((m == v).astype(np.uint8), out_hw) for v in VALUES])
        im = Image.fromarray(m, mode="P")
        im.putpalette(ic.PALETTE)
        out[f"{name}/ids"] = m
        out[f"{name}/masks"] = planes
        out[f"{name}/boxes"] = pc.any_boxes(planes).astype(np.int32)
        out[f"{name}/resized_ids"] = np.asarray(im.resize((out_hw[1], out_hw[0]), Image.NEAREST))
    recipe = {"pillow": PIL.__version__, "cases": [ic.case_id(c) for c in ic.GOLDEN_CASES], "values": list(VALUES)}
    out["recipe"] = np.frombuffer(json.dumps(recipe).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "g37_vos_folders_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
