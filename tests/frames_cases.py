"""Shared by the frame-resize tests and tools/gen_golden_frames.py: the cases and their closed-form inputs."""
import numpy as np

from univs_amd import synth

# (T, Hi, Wi) -> (Ho, Wo): what each exercises
CASES = [
    ((1, 37, 53), (20, 29)),      # odd down-scale, Wo % 4 != 0
    ((2, 37, 53), (74, 106)),     # exact 2x up, two frames
    ((1, 37, 53), (37, 29)),      # vertical identity
    ((1, 37, 53), (11, 53)),      # horizontal identity
    ((1, 5, 7), (64, 96)),        # border taps clipped to one
    ((3, 1, 9), (3, 4)),          # one input row
    ((1, 90, 160), (45, 80)),     # exact 2x down
    ((1, 97, 131), (64, 86)),     # 1.5x
    ((2, 135, 240), (90, 160)),   # the 1080p -> 720p ratio
    ((1, 33, 47), (100, 141)),    # 3x up
    ((1, 150, 260), (100, 173)),  # several tiles on both axes, ragged last tile
    ((1, 131, 97), (86, 64)),     # portrait
    ((1, 96, 128), (24, 32)),     # scale 4, the coverage edge
]
UNCOVERED = [((1, 64, 96), (5, 7)), ((1, 48, 64), (1, 1))]
KINDS = ("noise", "binary", "ramp")
# tests/golden/g32_frames_pil.npz (tools/gen_golden_frames.py): one small frame per path of the rule, Pillow's bytes stored
GOLDEN_CASES = [
    ((1, 37, 53), (20, 29)), ((1, 37, 53), (37, 29)), ((1, 37, 53), (11, 53)), ((1, 1, 9), (3, 4)), ((1, 30, 52), (15, 26)),
    ((1, 33, 47), (22, 31)), ((1, 11, 15), (33, 45)), ((1, 5, 7), (24, 36)), ((1, 48, 64), (12, 16)), ((1, 64, 96), (5, 7)),
    ((1, 48, 64), (1, 1)),
]


def case_id(case):
    (T, Hi, Wi), (Ho, Wo) = case
    return f"{T}x{Hi}x{Wi}-{Ho}x{Wo}"


def frames(kind, T, H, W):
    """uint8 [T, H, W, 3]: uniform noise, 0 / 255 noise, or a ramp, from the project's closed-form hash (every machine makes the same)."""
    n = T * H * W * 3
    if kind == "noise":
        v = np.floor(synth.hash_u01(f"frames_resize/noise/{T}x{H}x{W}", n) * 256.0)
    elif kind == "binary":
        v = (synth.hash_u01(f"frames_resize/binary/{T}x{H}x{W}", n) < 0.5) * 255.0
    elif kind == "ramp":
        v = np.arange(n) % 256
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(np.asarray(v).reshape(T, H, W, 3).astype(np.uint8))
