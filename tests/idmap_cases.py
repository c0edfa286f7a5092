"""Shared by the id-map prompt tests and tools/gen_golden_vos_folders.py: closed-form id maps, the per-object references (Pillow itself
and numpy's `bincount` / `any`) and the small VOS data sets in the data sets' own folder layouts."""
import json
import os

import numpy as np

from tests import prompt_masks_cases as pc
from univs_amd import synth

# tests/golden/g37_vos_folders_pil.npz (tools/gen_golden_vos_folders.py): (H, W) -> (Ho, Wo), Pillow's bytes per value and the boxes stored
GOLDEN_CASES = [((2, 2), (7, 7)), ((7, 7), (2, 2)), ((37, 53), (20, 29)), ((37, 53), (74, 106))]


def case_id(case):
    (H, W), (Ho, Wo) = case
    return f"{H}x{W}-{Ho}x{Wo}"


def idmap(kind, H, W, values=(0, 1, 2, 255), seed=0):
    """uint8 [H, W] from the project's closed-form hash: "noise" draws every pixel from `values`, "regions" paints one rectangle per
    value (in order, later ones on top) on a ground of values[0]."""
    values = list(values)
    if kind == "noise":
        u = synth.hash_u01(f"idmap/noise/{H}x{W}/{seed}", H * W).reshape(H, W)
        return np.asarray(values, np.uint8)[np.minimum((u * len(values)).astype(np.int64), len(values) - 1)]
    if kind == "regions":
        m = np.full((H, W), values[0], np.uint8)
        u = synth.hash_u01(f"idmap/regions/{H}x{W}/{seed}", 4 * len(values)).reshape(-1, 4)
        for v, (a, b, c, d) in zip(values[1:], u):
            y0, x0 = int(a * H * 0.7), int(b * W * 0.7)
            m[y0:y0 + 1 + int(c * H * 0.5), x0:x0 + 1 + int(d * W * 0.5)] = v
        return m
    raise ValueError(kind)


def pillow_prompts(ids, frame, value, out_hw):
    """(uint8 [N, Ho, Wo], int64 [N, 4]): per listed object Pillow's NEAREST resize of its own plane, and the boxes by `any`."""
    want = np.stack([pc.pillow_resize((ids[f] == v).astype(np.uint8), out_hw) for f, v in zip(frame, value)]) if len(frame) else \
        np.zeros((0,) + tuple(out_hw), np.uint8)
    return want, pc.any_boxes(want)


def numpy_census(ids):
    """(count [F, 256], box [F, 256, 4]) by `bincount` and, per value, `any` over the rows and columns of its plane."""
    F = ids.shape[0]
    count, box = np.zeros((F, 256), np.int64), np.zeros((F, 256, 4), np.int64)
    for f in range(F):
        count[f] = np.bincount(ids[f].reshape(-1), minlength=256)
        box[f] = pc.any_boxes(np.stack([ids[f] == v for v in range(256)]))
    return count, box


# ---- the small data sets of the folder tests ---------------------------------------------------------------------------------------------
FH, FW = 12, 16
PALETTE = [0, 0, 0, 128, 0, 0, 0, 128, 0, 128, 128, 0] + [7] * (756 - 3) + [255, 255, 255]


def save_idmap(path, m, mode="P"):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if mode == "P":
        im = Image.fromarray(m, mode="P")
        im.putpalette(PALETTE)
        im.save(path)
    elif mode == "L":
        Image.fromarray(m, mode="L").save(path)
    elif mode == "P1":                                               # a palette file at bit depth 1 (values 0 / 1)
        im = Image.fromarray(m, mode="P")
        im.putpalette(PALETTE[:6])
        im.save(path, bits=1)
    else:
        raise ValueError(mode)


def save_frames(folder, names, hw=(FH, FW), seed=0):
    """Frames `names` (png or jpg by their extension) of noise at `hw`."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i, name in enumerate(names):
        u = synth.hash_u01(f"idmap/frames/{seed}/{i}", hw[0] * hw[1] * 3).reshape(hw[0], hw[1], 3)
        Image.fromarray((u * 255).astype(np.uint8)).save(os.path.join(folder, name))


def box_of(m):
    """The converters' `bounding_box` (convert_mose_to_cocovid_val.py:29-34), by their recipe: [x0, y0, x1 - x0, y1 - y0]."""
    ys, xs = np.flatnonzero(m.any(1)), np.flatnonzero(m.any(0))
    return [int(xs[0]), int(ys[0]), int(xs[-1] - xs[0]), int(ys[-1] - ys[0])]


def annotation(vid, obj, frames_maps, n_frames, **extra):
    """One annotation of the converters' json: `frames_maps` {frame index: id map} are the files the rule reads, the object is value
    `obj` in them."""
    segms, boxes = [None] * n_frames, [None] * n_frames
    for f, m in frames_maps.items():
        if (m == obj).any():
            segms[f] = pc.code_of((m == obj).astype(np.uint8))
            boxes[f] = box_of(m == obj)
    return {"video_id": vid, "iscrowd": 0, "segmentations": segms, "bboxes": boxes, **extra}


def write_json(path, videos, annotations):
    with open(path, "w") as f:
        json.dump({"videos": videos, "annotations": annotations, "categories": [{"supercategory": "object", "id": 1, "name": "object"}]}, f)
    return path


def video_entry(vid, names, hw=(FH, FW)):
    return {"id": vid, "file_names": [f"{vid}/{n}" for n in names], "height": hw[0], "width": hw[1], "length": len(names)}


def write_davis(root):
    """<root>/JPEGImages and <root>/Annotations in the DAVIS / MOSE layout and the json the MOSE converter's rule gives for them: video
    "bear" (3 frames; first annotation with values 0, 1, 2, 255; a later annotation with value 3, which the rule never reads), video
    "cat" (2 frames of 13 x 16, one object), "dog" without annotations (skipped).  Returns (json, image root, mask root)."""
    im_root, an_root = os.path.join(root, "JPEGImages"), os.path.join(root, "Annotations")
    names = ["00000.png", "00001.png", "00002.png"]
    save_frames(os.path.join(im_root, "bear"), names)
    save_frames(os.path.join(im_root, "cat"), names[:2], (FH + 1, FW), seed=1)
    save_frames(os.path.join(im_root, "dog"), names[:1], seed=2)
    bear0, bear2 = idmap("regions", FH, FW, (0, 1, 2, 255)), idmap("regions", FH, FW, (0, 3), seed=5)
    cat0 = idmap("regions", FH + 1, FW, (0, 4), seed=3)
    save_idmap(os.path.join(an_root, "bear", "00000.png"), bear0)
    save_idmap(os.path.join(an_root, "bear", "00002.png"), bear2)
    save_idmap(os.path.join(an_root, "cat", "00000.png"), cat0)
    annos = []
    for vid, m, n in (("bear", bear0, 3), ("cat", cat0, 2)):
        for v in np.unique(m).tolist():
            if v:
                a = annotation(vid, v, {0: m}, n, id=v, category_id=1)
                a["bboxes"] = [None] * n                             # (the MOSE converter stores the areas only)
                annos.append(a)
    videos = [video_entry("bear", names), video_entry("cat", names[:2], (FH + 1, FW))]
    return write_json(os.path.join(root, "davis.json"), videos, annos), im_root, an_root


def write_ytvos(root):
    """The YouTube-VOS layout with meta.json: video "zz" first in the meta (objects "2" and "1" in that order; object 1 appears only in
    the later annotated frame; a value 9 that is not in the meta) and video "aa" (object "5", and a meta object "6" that never occurs).
    Frames are jpg, annotations exist for some frames only."""
    im_root, an_root = os.path.join(root, "JPEGImages"), os.path.join(root, "Annotations")
    names = ["00000.jpg", "00005.jpg", "00010.jpg"]
    save_frames(os.path.join(im_root, "zz"), names)
    save_frames(os.path.join(im_root, "aa"), names[:2], seed=1)
    zz0, zz2 = idmap("regions", FH, FW, (0, 2, 9)), idmap("regions", FH, FW, (0, 2, 1), seed=4)
    aa0 = idmap("regions", FH, FW, (0, 5), seed=6)
    save_idmap(os.path.join(an_root, "zz", "00000.png"), zz0)
    save_idmap(os.path.join(an_root, "zz", "00010.png"), zz2)
    save_idmap(os.path.join(an_root, "aa", "00000.png"), aa0)
    meta = {"videos": {"zz": {"objects": {"2": {"category": "a", "frames": ["00000"]}, "1": {"category": "b", "frames": ["00010"]}}},
                       "aa": {"objects": {"5": {"category": "c", "frames": ["00000"]}, "6": {"category": "d", "frames": ["00000"]}}}}}
    with open(os.path.join(root, "meta.json"), "w") as f:
        json.dump(meta, f)
    annos = [annotation("zz", 2, {0: zz0, 2: zz2}, 3, id=1, ori_id="2", category_id=1),
             annotation("zz", 1, {0: zz0, 2: zz2}, 3, id=2, ori_id="1", category_id=1),
             annotation("aa", 5, {0: aa0}, 2, id=3, ori_id="5", category_id=1),
             annotation("aa", 6, {0: aa0}, 2, id=4, ori_id="6", category_id=1)]
    videos = [video_entry("zz", names), video_entry("aa", names[:2])]
    return write_json(os.path.join(root, "ytvos.json"), videos, annos), im_root, an_root


def write_viposeg(root, n_videos=1):
    """The VIPOSeg layout with meta.json and obj_class.json: video "v0" whose objects "1" (frames 00001 ..) and "7" (first frame 00003)
    have different label files, a value 4 that is not in the meta, grey ("L") label files; further videos "v1" .. are copies of a
    one-object video, for the dev prefixes."""
    im_root, an_root = os.path.join(root, "JPEGImages"), os.path.join(root, "Annotations")
    meta, classes, videos, annos = {"videos": {}}, {}, [], []
    for k in range(n_videos):
        vid = f"v{k}"
        if k == 0:
            frames = {"1": ["00001", "00002", "00003"], "7": ["00003", "00004"]}
            maps = {"00001": idmap("regions", FH, FW, (0, 1, 4)), "00003": idmap("regions", FH, FW, (0, 1, 7), seed=8)}
            classes[vid] = {"1": 12, "7": 3}
        else:
            frames = {"2": ["00000", "00001"]}
            maps = {"00000": idmap("regions", FH, FW, (0, 2), seed=10 + k)}
            classes[vid] = {"2": 40 + k}
        meta["videos"][vid] = {"objects": {key: {"frames": fr} for key, fr in frames.items()}}
        names = sorted({n + ".jpg" for fr in frames.values() for n in fr})
        save_frames(os.path.join(im_root, vid), names, seed=k)
        for stem, m in maps.items():
            save_idmap(os.path.join(an_root, vid, stem + ".png"), m, mode="L")
        by_frame = {names.index(stem + ".jpg"): m for stem, m in maps.items()}
        for key in frames:
            annos.append(annotation(vid, int(key), by_frame, len(names), id=int(key), category_id=classes[vid][key]))
        videos.append(video_entry(vid, names))
    with open(os.path.join(root, "meta.json"), "w") as f:
        json.dump(meta, f)
    with open(os.path.join(root, "obj_class.json"), "w") as f:
        json.dump(classes, f)
    return write_json(os.path.join(root, "viposeg.json"), videos, annos), im_root, an_root
