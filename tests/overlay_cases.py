"""Scenes for the overlay tests (tests/test_overlay_rule_cpu.py, test_overlay_jpeg_gpu.py): id maps whose objects touch every image side and
each other, with ids below 0 and beyond the table, and the folder and model of a `python -m univs_amd.run --visualize` run."""
import os

import numpy as np
import torch
from PIL import Image

from tests import cases
from tests.jpeg_cases import content

SIZES = ((40, 48), (75, 131))                                        # (H, W)
LUT = np.array([[0, 0, 0, 0], [220, 20, 60, 128], [0, 200, 0, 255], [10, 10, 250, 204], [255, 255, 0, 1], [90, 90, 90, 153]], np.uint8)


def scene(H, W, T=3, seed=0):
    """(frames uint8 [T, H, W, 3], ids int64 [T, H, W]): object 1 fills the top-left corner, 2 the bottom-right one, 3 a band that touches
    both and the left and right sides, 4 a single pixel, 5 a block of ids beyond the table (99), and a block of negative ids."""
    frames = np.stack([content(("noise", "smooth", "patches")[t % 3], H, W, 5000 + seed + t) for t in range(T)])
    ids = np.zeros((T, H, W), np.int64)
    for t in range(T):
        ids[t, :H // 3, :W // 3 + t] = 1
        ids[t, H // 2:, W // 2 - t:] = 2
        ids[t, H // 3:H // 2, :] = 3
        ids[t, 2, W - 3] = 4
        ids[t, H - 6:H - 3, 2:7] = 99
        ids[t, 1:4, W // 2:W // 2 + 3] = -7
    return frames, ids


def write_videos(root, n_videos=2, n_frames=5, H=32, W=40):
    """A folder of `n_videos` sub-folders of `n_frames` JPEG frames."""
    for v in range(n_videos):
        os.makedirs(os.path.join(root, f"video{v}"))
        for f in range(n_frames):
            Image.fromarray(content("smooth", H, W, 5100 + 10 * v + f)).save(os.path.join(root, f"video{v}", f"{f:05d}.jpg"), quality=90)


def write_model(root, entities="vss"):
    """(config file, weights) of a small synthetic UniVS_Prompt whose custom-video mode runs the entity driver's `entities` sub-task."""
    from univs_amd import synth
    from univs_amd.config import load_cfg
    from univs_amd.modeling.build import build_model
    torch.save(cases.clip_table(), os.path.join(root, "clip.pt"))
    cfg = os.path.join(root, "cfg.yaml")
    with open(cfg, "w") as f:
        f.write(f"""MODEL:
  META_ARCHITECTURE: UniVS_Prompt
  MASK_FORMER:
    NUM_OBJECT_QUERIES: 20
  UniVS:
    CLIP_CLASS_EMBED_PATH: {os.path.join(root, "clip.pt")}
    TEST:
      VIDEO_UNIFIED_INFERENCE_ENABLE: True
      VIDEO_UNIFIED_INFERENCE_ENTITIES: {entities}
      CUSTOM_VIDEOS_ENABLE: True
INPUT:
  SAMPLING_FRAME_NUM: 2
  MIN_SIZE_TEST: 32
  MAX_SIZE_TEST: 64
""")
    model = build_model(load_cfg(cfg)).eval()
    synth.load_synthetic(model)
    torch.save({"model": model.state_dict()}, os.path.join(root, "w.pth"))
    return cfg, os.path.join(root, "w.pth")
