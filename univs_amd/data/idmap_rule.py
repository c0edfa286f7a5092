"""The two entries of include/univs_idmap_hip.h in numpy: the statement csrc/idmap_prompts.hip is held to, and the CPU path of the
tests (tests/test_idmap_rule_cpu.py pins it to Pillow itself, to numpy's `bincount` / `any` and to tests/golden/g37_vos_folders_pil.npz).

An id map is uint8 [H, W]: the pixels of an indexed annotation PNG, a pixel's value is its object's id.  Pillow's NEAREST resize is a
gather, out[yo, xo] = in[ty[yo], tx[xo]] with the tables of resize_rule.py, so `resize(idmap) == v` equals `resize(idmap == v)` for
every value v: one gather of the id map gives the resized plane of every object.  Pure numpy, no torch.
"""
import numpy as np

from .resize_rule import nearest_table


def _ids(ids):
    ids = np.asarray(ids)
    if ids.dtype != np.uint8 or ids.ndim != 3:
        raise ValueError(f"idmap_rule: uint8 [F, H, W] id maps, got {ids.dtype} {ids.shape}")
    return ids


def plane_boxes(planes):
    """int32 [n, 4] = {x0, y0, x1 + 1, y1 + 1} of the first / last true column and row of bool [n, h, w], zeros for an empty plane."""
    planes = np.asarray(planes).astype(bool)
    out = np.zeros((planes.shape[0], 4), np.int32)
    for i, m in enumerate(planes):
        xs, ys = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
        if xs.size:
            out[i] = (xs[0], ys[0], xs[-1] + 1, ys[-1] + 1)
    return out


def census(ids):
    """(count int32 [F, 256], box int32 [F, 256, 4]) of uint8 [F, H, W]: per frame and value the number of pixels and
    {x0, y0, x1 + 1, y1 + 1} at the source size, zeros for a value that is absent (`univs_idmap_census_u8`)."""
    ids = _ids(ids)
    F = ids.shape[0]
    count = np.zeros((F, 256), np.int32)
    box = np.zeros((F, 256, 4), np.int32)
    ys, xs = np.nonzero(np.ones(ids.shape[1:], bool))                # every pixel's row and column
    for f in range(F):
        v = ids[f].reshape(-1).astype(np.int64)
        count[f] = np.bincount(v, minlength=256)
        x0, y0 = np.full(256, np.iinfo(np.int32).max, np.int64), np.full(256, np.iinfo(np.int32).max, np.int64)
        x1, y1 = np.full(256, -1, np.int64), np.full(256, -1, np.int64)
        np.minimum.at(x0, v, xs)
        np.minimum.at(y0, v, ys)
        np.maximum.at(x1, v, xs)
        np.maximum.at(y1, v, ys)
        have = count[f] > 0
        box[f, have] = np.stack([x0, y0, x1 + 1, y1 + 1], 1)[have]
    return count, box


def prompts(ids, frame, value, ty, tx):
    """(masks uint8 [N, Ho, Wo], boxes int32 [N, 4]) of `univs_idmap_prompts_u8`: masks[n] = (ids[frame[n]][ty][:, tx] == value[n])
    and its box; frame is clamped to [0, F), value to [0, 255], the table entries to the source."""
    ids = _ids(ids)
    F, H, W = ids.shape
    frame, value = np.asarray(frame, np.int64).reshape(-1), np.asarray(value, np.int64).reshape(-1)
    ty, tx = np.clip(np.asarray(ty, np.int64), 0, H - 1), np.clip(np.asarray(tx, np.int64), 0, W - 1)
    masks = np.zeros((len(frame), len(ty), len(tx)), np.uint8)
    if len(frame) and F < 1:
        raise ValueError("idmap_rule.prompts: objects listed, but no frame")
    for n, (f, v) in enumerate(zip(np.clip(frame, 0, F - 1), np.clip(value, 0, 255))):
        masks[n] = ids[f][ty][:, tx] == v
    return masks, plane_boxes(masks)


def prompts_resized(ids, frame, value, out_hw):
    """`prompts` with Pillow's NEAREST tables for (Ho, Wo) = out_hw: what the mapper asks for."""
    ids = _ids(ids)
    return prompts(ids, frame, value, nearest_table(ids.shape[1], out_hw[0]), nearest_table(ids.shape[2], out_hw[1]))


def converter_box(box):
    """[x0, y0, x1 - x0, y1 - y0] of a census box {x0, y0, x1 + 1, y1 + 1}: the `bounding_box` of the reference's converters
    (convert_mose_to_cocovid_val.py:29-34), whose width and height are one short of the pixels covered -- kept as it is."""
    x0, y0, x1p, y1p = (int(v) for v in box)
    return [x0, y0, x1p - 1 - x0, y1p - 1 - y0]
