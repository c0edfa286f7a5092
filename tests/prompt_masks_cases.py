"""Shared by the first-frame-mask tests and tools/gen_golden_prompts.py: closed-form masks, their run-length codes, the references
(Pillow and the torch box rule) and the small VOS data set the mapper tests write to disk."""
import json
import os

import numpy as np
import torch

from univs_amd import synth

# tests/golden/g33_prompt_masks_pil.npz (tools/gen_golden_prompts.py): (kind, H, W) -> (Ho, Wo), Pillow's bytes and the boxes stored
GOLDEN_CASES = [
    (("noise", 2, 2), (7, 7)), (("noise", 7, 7), (2, 2)), (("blob", 37, 53), (20, 29)), (("blob", 37, 53), (74, 106)),
    (("noise", 1, 9), (3, 4)), (("checker", 5, 7), (24, 36)), (("full", 4, 6), (3, 5)), (("empty", 4, 6), (8, 3)),
    (("last", 9, 5), (9, 5)),
]


def case_id(case):
    (kind, H, W), (Ho, Wo) = case
    return f"{kind}-{H}x{W}-{Ho}x{Wo}"


def mask(kind, H, W, seed=0):
    """uint8 [H, W] of 0 / 1 from the project's closed-form hash (every machine makes the same)."""
    if kind == "noise":
        m = synth.hash_u01(f"prompt_masks/noise/{H}x{W}/{seed}", H * W).reshape(H, W) < 0.5
    elif kind == "blob":                                             # a few rectangles: long runs, whole columns without a boundary
        m = np.zeros((H, W), bool)
        u = synth.hash_u01(f"prompt_masks/blob/{H}x{W}/{seed}", 12).reshape(3, 4)
        for a, b, c, d in u:
            y0, x0 = int(a * H * 0.7), int(b * W * 0.7)
            m[y0:y0 + 1 + int(c * H * 0.4), x0:x0 + 1 + int(d * W * 0.4)] = True
    elif kind == "checker":                                          # H W runs for an odd H (an even one joins runs across columns)
        m = (np.add.outer(np.arange(H), np.arange(W)) % 2) == 1
    elif kind == "full":                                             # an empty first run
        m = np.ones((H, W), bool)
    elif kind == "empty":                                            # one run
        m = np.zeros((H, W), bool)
    elif kind == "last":                                             # foreground ending on the last pixel
        m = np.zeros((H, W), bool)
        m[H // 2:, W - 1] = True
    elif kind == "span":                                             # one run spanning several source columns
        m = np.zeros((H, W), bool)
        m[H // 2:, 1] = True
        m[:, 2:W - 2] = True
        m[:H // 3, W - 2] = True
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(m.astype(np.uint8))


def counts_of(m):
    """The uncompressed COCO counts (a list of ints, the first a run of zeros) of a 0 / 1 mask [H, W]."""
    flat = np.asarray(m, dtype=np.uint8).T.reshape(-1)
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [flat.shape[0]]])
    counts = np.diff(edges).tolist()
    return ([0] if flat[0] else []) + counts


def code_of(m, compressed=False):
    """{"size", "counts"} of a 0 / 1 mask: a list of counts, or the compressed string."""
    if compressed:
        from univs_amd.inference.results import rle_encode_masks
        return rle_encode_masks(torch.from_numpy(np.asarray(m)))[0]
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": counts_of(m)}


def pillow_resize(m, out_hw):
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(m, dtype=np.uint8)).resize((out_hw[1], out_hw[0]), Image.NEAREST))


def any_boxes(masks):
    """int64 [n, 4] of 0 / 1 masks [n, h, w]: the first and last true column and row as [x0, y0, x1 + 1, y1 + 1], zeros for an empty
    mask -- detectron2's `BitMasks.get_bounding_boxes`, written out with `any`."""
    masks = np.asarray(masks).astype(bool)
    out = np.zeros((masks.shape[0], 4), np.int64)
    for i, m in enumerate(masks):
        xs, ys = np.flatnonzero(m.any(0)), np.flatnonzero(m.any(1))
        if xs.size and ys.size:
            out[i] = [xs[0], ys[0], xs[-1] + 1, ys[-1] + 1]
    return out


# ---- the small VOS data set of the mapper tests ----------------------------------------------------------------------------------------
VOS_H, VOS_W, VOS_N = 37, 53, 4


def write_vos_dataset(root):
    """<root>/JPEGImages/<video>/<frame>.png for two videos, <root>/Annotations/a/00000.png with a palette, and <root>/vos.json:
    video 5 ("a": three objects -- one with `ori_id`, given as a list of counts; one without, given as a compressed string, that is
    annotated again in frame 2; one that enters at frame 2 -- an `iscrowd` object, and a `None` frame) and video 2 ("b", 38 rows, one
    object, frame 0).  Returns (json path, image root, {(video id, frame): {object id: uint8 [H, W]}})."""
    from PIL import Image
    from tests.frames_cases import frames
    image_root = os.path.join(root, "JPEGImages")
    for k, name in enumerate(("a", "b")):
        os.makedirs(os.path.join(image_root, name))
        for i, f in enumerate(frames("noise", VOS_N, VOS_H + k, VOS_W)):
            Image.fromarray(f).save(os.path.join(image_root, name, f"{i:05d}.png"))
    os.makedirs(os.path.join(root, "Annotations", "a"))
    im = Image.fromarray(np.zeros((VOS_H, VOS_W), np.uint8), mode="P")
    im.putpalette([0, 0, 0, 128, 0, 0, 0, 128, 0] + [0] * 759)
    im.save(os.path.join(root, "Annotations", "a", "00000.png"))
    truth = {(5, 0): {1: mask("blob", VOS_H, VOS_W, 1), 2: mask("noise", VOS_H, VOS_W, 2), 9: mask("blob", VOS_H, VOS_W, 9)},
             (5, 2): {2: mask("blob", VOS_H, VOS_W, 3), 3: mask("span", VOS_H, VOS_W)},
             (2, 0): {4: mask("blob", VOS_H + 1, VOS_W, 4)}}
    none = [None] * VOS_N

    def segms(vid, oid, compressed):
        return [code_of(truth[vid, f][oid], compressed) if oid in truth.get((vid, f), {}) else None for f in range(VOS_N)]

    def boxes(vid, oid):
        return [[1, 2, 3, 4] if oid in truth.get((vid, f), {}) else None for f in range(VOS_N)]

    annotations = [
        {"id": 1, "video_id": 5, "category_id": 7, "iscrowd": 0, "ori_id": 41, "segmentations": segms(5, 1, False), "bboxes": boxes(5, 1)},
        {"id": 2, "video_id": 5, "category_id": 3, "iscrowd": 0, "segmentations": segms(5, 2, True), "bboxes": boxes(5, 2)},
        {"id": 3, "video_id": 5, "category_id": 7, "iscrowd": 0, "ori_id": 43, "segmentations": segms(5, 3, False), "bboxes": boxes(5, 3)},
        {"id": 9, "video_id": 5, "category_id": 3, "iscrowd": 1, "segmentations": segms(5, 9, True), "bboxes": boxes(5, 9)},
        {"id": 8, "video_id": 5, "category_id": 3, "iscrowd": 0, "segmentations": none, "bboxes": none},
        {"id": 4, "video_id": 2, "category_id": 3, "iscrowd": 0, "segmentations": segms(2, 4, True), "bboxes": boxes(2, 4)},
    ]
    videos = [{"id": 5, "file_names": [f"a/{i:05d}.png" for i in range(VOS_N)], "height": VOS_H, "width": VOS_W, "length": VOS_N},
              {"id": 2, "file_names": [f"b/{i:05d}.png" for i in range(VOS_N)], "height": VOS_H + 1, "width": VOS_W, "length": VOS_N}]
    data = {"videos": videos, "annotations": annotations, "categories": [{"id": 3, "name": "x"}, {"id": 7, "name": "y"}]}
    path = os.path.join(root, "vos.json")
    with open(path, "w") as f:
        json.dump(data, f)
    return path, image_root, truth
