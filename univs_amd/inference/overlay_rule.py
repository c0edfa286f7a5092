"""The overlay of a result on its frame, stated once in numpy: the yardstick of the overlay path of csrc/jpeg_encode.hip.  No GPU (but
`idmap_from_instances`, which is torch on the masks' device).

The reference draws its custom-video pictures with matplotlib (univs/inference/inference_video_entity.py:1134-1322: text labels,
jittered colours, anti-aliased polygons); none of that is reproducible bit for bit and none of it is attempted.  This rule is the
project's own, as the result-PNG format and the HOTA protocol are:

  inputs   frame uint8 [H, W, 3]: the file's own pixels at the output size (the reference re-interpolates the model input with
           F.interpolate(...).long() instead); ids integer [H, W]; lut uint8 [K, 4] = (r, g, b, alpha); edge (r, g, b) or None
  pixel    k = min(max(ids, 0), K - 1), a = lut[k, 3], out_c = (frame_c (255 - a) + lut[k, c] a + 127) // 255; where `edge` is given,
           a > 0 and a 4-neighbour *inside the image* has another clamped id, out = edge

  lut_from_palette(palette, alpha)        VOS: the PNG palette's colours, id 0 transparent
  lut_from_categories(categories, alpha)  VPS / VSS: row 0 transparent, row 1 + k the k-th category (sorted by id) in its dataset colour
  idmap_from_instances(masks, scores)     VIS: a pixel's id is 1 + the index of the highest-scored kept instance covering it
"""
import numpy as np
import torch

OFF_WHITE = (255, 255, 240)                                          # the reference's _OFF_WHITE: the contour colour
ALPHA_VOS, ALPHA_VPS, ALPHA_VSS = 128, 204, 153                      # the reference's 0.8 (VPS) and 0.6 (VSS) of 255


def check_lut(lut):
    lut = np.asarray(lut)
    if lut.ndim != 2 or lut.shape[1] != 4 or lut.shape[0] < 1 or lut.dtype != np.uint8:
        raise ValueError(f"lut: uint8 [K, 4] with K >= 1, got {lut.dtype} {tuple(lut.shape)}")
    return lut


def check_edge(edge):
    """None, or the three channel values as ints."""
    if edge is None:
        return None
    edge = tuple(int(c) for c in edge)
    if len(edge) != 3 or not all(0 <= c <= 255 for c in edge):
        raise ValueError(f"edge={edge!r}: (r, g, b) of 0..255, or None")
    return edge


def overlay_rule(frame, ids, lut, edge=OFF_WHITE):
    """uint8 [H, W, 3]."""
    frame, ids, lut, edge = np.asarray(frame), np.asarray(ids), check_lut(lut), check_edge(edge)
    if frame.ndim != 3 or frame.shape[2] != 3 or frame.dtype != np.uint8 or ids.shape != frame.shape[:2] or ids.dtype.kind not in "iu":
        raise ValueError(f"frame uint8 [H, W, 3] and integer ids [H, W], got {frame.dtype} {tuple(frame.shape)} and {ids.dtype} {tuple(ids.shape)}")
    k = np.clip(ids.astype(np.int64), 0, lut.shape[0] - 1)
    a = lut[k, 3].astype(np.int64)[:, :, None]
    out = ((frame.astype(np.int64) * (255 - a) + lut[k, :3].astype(np.int64) * a + 127) // 255).astype(np.uint8)
    if edge is not None:
        differs = np.zeros(k.shape, bool)
        differs[1:] |= k[1:] != k[:-1]
        differs[:-1] |= k[:-1] != k[1:]
        differs[:, 1:] |= k[:, 1:] != k[:, :-1]
        differs[:, :-1] |= k[:, :-1] != k[:, 1:]
        out[differs & (a[:, :, 0] > 0)] = edge
    return out


def default_palette(n=256):
    """The PASCAL VOC colour map (the DAVIS palette), uint8 [n, 3]: what a result without a palette or category colours is drawn with."""
    pal = np.zeros((n, 3), np.uint8)
    for i in range(n):
        c = i
        for j in range(8):
            pal[i] |= np.array([(c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1], np.uint8) << (7 - j)
            c >>= 3
    return pal


def lut_from_palette(palette, alpha=ALPHA_VOS):
    """uint8 [K, 4] of a PNG palette (a flat list or array of r, g, b, ...): id k in its colour, id 0 transparent."""
    pal = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    lut = np.concatenate([pal, np.full((len(pal), 1), int(alpha), np.uint8)], axis=1)
    lut[0, 3] = 0
    return lut


def lut_from_categories(categories, alpha=ALPHA_VPS):
    """(uint8 [1 + C, 4], [category id per row, None for row 0]) of {category id: {"color": (r, g, b), ...}}: the colours
    `write_vps_predictions` paints a category's first segment with."""
    order = sorted(categories)
    lut = np.zeros((len(order) + 1, 4), np.uint8)
    for row, cid in enumerate(order, 1):
        lut[row, :3] = np.asarray(categories[cid]["color"], dtype=np.uint8)
        lut[row, 3] = int(alpha)
    return lut, [None] + order


def idmap_from_instances(masks, scores, score_thresh=0.02):
    """int32 [T, H, W] on the masks' device, of bool masks [N, T, H, W] and scores [N]: 1 + the index of the highest-scored instance
    with score >= score_thresh that covers the pixel (ties: the lower index), 0 where none does."""
    masks = torch.as_tensor(masks)
    scores = torch.as_tensor(scores, dtype=torch.float32, device=masks.device)
    if masks.ndim != 4 or scores.shape != (masks.shape[0],):
        raise ValueError(f"masks [N, T, H, W] and scores [N], got {tuple(masks.shape)} and {tuple(scores.shape)}")
    out = torch.zeros(masks.shape[1:], dtype=torch.int32, device=masks.device)
    kept = (scores >= score_thresh).tolist()                         # (compared as float32, as the scores are)
    keep = [i for i in torch.argsort(scores, descending=True, stable=True).tolist() if kept[i]]
    for i in reversed(keep):                                         # painted from the lowest kept score up: the best is on top
        out[masks[i].bool()] = i + 1
    return out
