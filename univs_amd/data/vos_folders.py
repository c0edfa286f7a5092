"""The records of a video-object-segmentation data set straight from the folders it ships as -- `JPEGImages/<video>/*.jpg` beside
`Annotations/<video>/*.png`, indexed PNGs whose pixel values are object ids -- without the detour through a YouTube-VIS json.

The reference reads such a data set only after one of its converter scripts (datasets/data_utils/convert_*_to_cocovid_val.py; they
need cv2, pycocotools and detectron2) has written that json; `vos_records_from_dirs` returns the records `load_vos_json` returns for the
json the converter would have written, with the video's folder name as its id and with one deliberate difference: where the json has
an object's `"segmentation"` (a run-length code of the plane `mask == obj_id`) the record has `{"png": path, "value": v}` -- the id map
and the value to compare it with.  `VOSTestMapper` makes the prompt masks from those (csrc/idmap_prompts.hip).  A record also carries
`"mask_files"`, the video's annotation PNGs sorted by name.

The converters' rules, restated (`dataset_name` chooses):

  sot_davis16* / sot_davis17* / mots_mose*  (convert_mose_to_cocovid_val.py:87-128; the reference has no DAVIS converter and registers
      DAVIS jsons of unknown origin -- that DAVIS follows the MOSE rule is this project's own statement)  The videos are the folders of
      image_root that mask_root has too.  Frames: the sorted listing.  Only the FIRST annotation PNG is read and it is taken as frame
      0's, so its stem has to be frame 0's (a ValueError otherwise).  Objects: its non-zero values in ascending order, `id` = the value,
      `category_id` 1, `iscrowd` 0, annotated in frame 0 only.  The converter computes a box but stores only the area: `bbox` is None.
  sot_ytbvos18*  (convert_ytvos_to_cocovid_val.py:63-111)  The videos and their objects are those of meta.json, `videos[v]["objects"]`
      in file order: `ori_id` = the key, `id` = a counter over the whole data set, `category_id` 1.  Every frame whose PNG (the frame's
      name with .jpg -> .png) exists annotates every object of the meta whose value occurs in it.
  pvos_viposeg*  (convert_viposeg_to_cocovid_val.py:80-148)  The videos are those of meta.json in file order -- the first tenth of them
      for a `*_dev` name, the first quarter for `*_dev0.25`, each rounded down.  Frames: the sorted union of the objects' `frames` lists,
      + ".jpg".  Label files: each object's first frame, + ".png".  `id` = int(key), `category_id` from obj_class.json; a label file
      annotates the objects of the meta whose value occurs in it, values that are not in the meta are skipped.
  mots_burst*  NotImplementedError: its native format is the json.

`bbox` is the converters' `bounding_box`, [x0, y0, x1 - x0, y1 - y0]: one short of the pixels covered, kept as it is.  The converters'
`areas` (that box's w h for MOSE and YouTube-VOS, the pixel count for VIPOSeg) are not part of a `load_vos_json` record, so they are not
part of these either; `idmap_rule.census` has both.  Which values occur where comes from that census: `reader="host"` opens each file
with Pillow by the converter's own expression and counts in numpy, `reader="gpu"` decodes the files on the device
(png_read_ops.read_pngs_device, one call per video; a file it does not take goes through the host expression) and counts there
(idmap_ops.idmap_census_u8): only the counts and boxes come down.
"""
import json
import os

import numpy as np
from PIL import Image

from . import idmap_rule
from .datasets import _SOT_PREFIXES, _record
from .images import read_image
from .vos_datasets import is_vos_name

_MOSE_RULE = ("sot_davis16", "sot_davis17", "mots_mose")
_YTVOS_RULE = ("sot_ytbvos18",)
_VIPOSEG_RULE = ("pvos_viposeg",)


def read_idmap(path, dataset_name=""):
    """uint8 [H, W] of an annotation PNG by the converter's own expression: `np.array(Image.open(f), dtype=np.uint8)` for VIPOSeg
    (convert_viposeg_to_cocovid_val.py:120-121), `np.array(Image.open(f).convert("P"))` for the others
    (convert_mose_to_cocovid_val.py:100-101)."""
    with Image.open(path) as im:
        if _VIPOSEG_RULE[0] in dataset_name:                         # (a record's name has "sot_" in front)
            return np.array(im, dtype=np.uint8)
        return np.array(im.convert("P"))


def _device_maps(paths, dataset_name, device):
    """The id maps of `paths` as device tensors: grey and palette files (colour type 0 or 3) through the device reader in one call,
    every other file -- and those the device does not take -- through the host expression."""
    import torch
    from .. import png_read_ops
    from ..inference import png_read
    datas = []
    for p in paths:
        with open(p, "rb") as f:
            datas.append(f.read())
    to_device = []
    for i, data in enumerate(datas):
        try:
            if png_read.parse_png(data).colour_type in (0, 3):
                to_device.append(i)
        except png_read.PngParseError:
            pass
    maps = [None] * len(paths)
    planes = png_read_ops.read_pngs_device([datas[i] for i in to_device], device, uncovered="host",
                                           host_reader=lambda k: read_idmap(paths[to_device[k]], dataset_name))
    for i, plane in zip(to_device, planes):
        maps[i] = plane
    for i, p in enumerate(paths):
        if maps[i] is None:
            maps[i] = torch.as_tensor(np.ascontiguousarray(read_idmap(p, dataset_name))).to(device)
    return maps


def census_of_files(paths, hw, dataset_name, video, reader="host", device=None):
    """(count [F, 256], box [F, 256, 4]) of the annotation PNGs `paths`, numpy on the host; a file whose size is not `hw` is a
    ValueError naming the video and the file."""
    def check(shape, path):
        if tuple(shape) != tuple(hw):
            raise ValueError(f"video {video}: annotation {path} is {tuple(shape)}, the video's frames are {tuple(hw)}")

    if not paths:
        return np.zeros((0, 256), np.int32), np.zeros((0, 256, 4), np.int32)
    if reader == "gpu":
        import torch
        from .. import idmap_ops
        maps = _device_maps(paths, dataset_name, torch.device("cuda" if device is None else device))
        for m, p in zip(maps, paths):
            check(m.shape, p)
        ids = torch.stack(maps)
        out = idmap_ops.idmap_census_u8(ids)
        if out is not None:
            return out[0].cpu().numpy(), out[1].cpu().numpy()
        return idmap_rule.census(ids.cpu().numpy())
    maps = [read_idmap(p, dataset_name) for p in paths]
    for m, p in zip(maps, paths):
        check(m.shape, p)
    return idmap_rule.census(np.stack(maps))


def _load_json(path, what):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"vos_records_from_dirs: {what} needs {path} (meta_dir defaults to the folder above the annotations)")
    with open(path) as f:
        return json.load(f)


def _pngs(folder):
    return [os.path.join(folder, n) for n in sorted(os.listdir(folder)) if n.lower().endswith(".png")] if os.path.isdir(folder) else []


def _new_record(image_root, mask_root, video, frames, dataset_name):
    paths = [os.path.join(image_root, video, n) for n in frames]
    height, width = read_image(paths[0]).shape[:2]                   # (as video_records_from_dir reads it)
    rec = _record(paths, height, width, video, "sot_" + dataset_name, "sot", has_mask=True)
    rec["mask_files"] = _pngs(os.path.join(mask_root, video))
    return rec


def _mose_records(image_root, mask_root, dataset_name, census):
    records = []
    for video in sorted(os.listdir(image_root)):
        if not os.path.isdir(os.path.join(image_root, video)) or not os.path.isdir(os.path.join(mask_root, video)):
            continue                                                 # (the converter skips a video without annotations)
        frames = sorted(os.listdir(os.path.join(image_root, video)))
        masks = sorted(os.listdir(os.path.join(mask_root, video)))
        if not frames:
            continue
        if not masks or os.path.splitext(masks[0])[0] != os.path.splitext(frames[0])[0]:
            raise ValueError(f"video {video}: its first annotation ({masks[0] if masks else 'none'}) is not that of its first frame "
                             f"({frames[0]}); the {dataset_name} rule reads the first annotation as frame 0's")
        rec = _new_record(image_root, mask_root, video, frames, dataset_name)
        png = os.path.join(mask_root, video, masks[0])
        count, _ = census([png], rec, video)
        for v in np.flatnonzero(count[0]).tolist():
            if v != 0:
                rec["annotations"][0].append({"iscrowd": 0, "category_id": 1, "id": v, "bbox": None, "png": png, "value": v})
        records.append(rec)
    return records


def _ytvos_records(image_root, mask_root, meta_dir, dataset_name, census):
    meta = _load_json(os.path.join(meta_dir, "meta.json"), dataset_name)["videos"]
    records, inst = [], 0
    for video, info in meta.items():
        frames = sorted(os.listdir(os.path.join(image_root, video)))
        rec = _new_record(image_root, mask_root, video, frames, dataset_name)
        objects = []
        for key in info["objects"]:
            inst += 1
            objects.append((key, inst))
        pngs = [os.path.join(mask_root, video, n.replace(".jpg", ".png")) for n in frames]
        annotated = [f for f, p in enumerate(pngs) if os.path.exists(p)]
        count, box = census([pngs[f] for f in annotated], rec, video)
        for k, f in enumerate(annotated):
            for key, inst_id in objects:
                v = int(key)
                if 0 <= v < 256 and count[k, v]:
                    rec["annotations"][f].append({"iscrowd": 0, "category_id": 1, "id": inst_id, "ori_id": key,
                                                  "bbox": idmap_rule.converter_box(box[k, v]), "png": pngs[f], "value": v})
        records.append(rec)
    return sorted(records, key=lambda r: r["video_id"])


def _viposeg_records(image_root, mask_root, meta_dir, dataset_name, census):
    meta = _load_json(os.path.join(meta_dir, "meta.json"), dataset_name)["videos"]
    classes = _load_json(os.path.join(meta_dir, "obj_class.json"), dataset_name)
    videos = list(meta)
    if dataset_name.startswith("pvos_viposeg_dev0.25"):
        videos = videos[:int(len(videos) * 0.25)]
    elif dataset_name.startswith("pvos_viposeg_dev"):
        videos = videos[:int(len(videos) * 0.1)]
    records = []
    for video in videos:
        objects = meta[video]["objects"]
        frames = sorted({name + ".jpg" for obj in objects.values() for name in obj["frames"]})
        labels = sorted({obj["frames"][0] + ".png" for obj in objects.values()})
        rec = _new_record(image_root, mask_root, video, frames, dataset_name)
        pngs = [os.path.join(mask_root, video, n) for n in labels]
        count, box = census(pngs, rec, video)
        for k, label in enumerate(labels):
            f = frames.index(label.replace(".png", ".jpg"))
            for key in objects:                                      # (a value that is not in the meta is never asked for)
                v = int(key)
                if 0 <= v < 256 and count[k, v]:
                    rec["annotations"][f].append({"iscrowd": 0, "category_id": classes[video][key], "id": v,
                                                  "bbox": idmap_rule.converter_box(box[k, v]), "png": pngs[k], "value": v})
        records.append(rec)
    return sorted(records, key=lambda r: r["video_id"])


def vos_records_from_dirs(image_root, mask_root, dataset_name, meta_dir=None, reader="host", device=None):
    """The records of `load_vos_json` for the VOS data set in image_root (`JPEGImages`) and mask_root (`Annotations`), by the rule of
    `dataset_name` (the module's docstring), videos in the order of their folder names.  meta_dir (meta.json, obj_class.json)
    defaults to the folder above mask_root, the data sets' own layout.  reader: who decodes and counts the annotation PNGs."""
    if not is_vos_name(dataset_name):
        raise ValueError(f"vos_records_from_dirs: {dataset_name!r} is no VOS data set (the names that begin with one of {_SOT_PREFIXES}); "
                         "data.video_records_from_dir reads a folder of frames without annotations")
    if reader not in ("host", "gpu"):
        raise ValueError(f"vos_records_from_dirs: reader={reader!r} (\"host\" or \"gpu\")")
    if dataset_name.startswith("mots_burst"):
        raise NotImplementedError(f"{dataset_name}: BURST ships its annotations as json, not as folders of PNGs; data.load_vos_json reads it")
    if meta_dir is None:
        meta_dir = os.path.dirname(os.path.abspath(mask_root))

    def census(paths, rec, video):
        return census_of_files(paths, (rec["height"], rec["width"]), dataset_name, video, reader=reader, device=device)

    if dataset_name.startswith(_MOSE_RULE):
        return _mose_records(image_root, mask_root, dataset_name, census)
    if dataset_name.startswith(_YTVOS_RULE):
        return _ytvos_records(image_root, mask_root, meta_dir, dataset_name, census)
    if dataset_name.startswith(_VIPOSEG_RULE):
        return _viposeg_records(image_root, mask_root, meta_dir, dataset_name, census)
    raise ValueError(f"vos_records_from_dirs: no folder rule for {dataset_name!r} (sot_davis16*, sot_davis17*, mots_mose*, sot_ytbvos18*, "
                     "pvos_viposeg*)")
