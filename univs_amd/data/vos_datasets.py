"""The records of a video-object-segmentation test file: `load_ytvis_json(..., sot=True)` (univs/data/datasets/ytvis.py:143-378),
without detectron2's catalog and the YTVOS api.  The splits registered that way are DAVIS, YouTube-VOS, MOSE, BURST and VIPOSeg
(`_SOT_PREFIXES` of datasets.py).

`record["annotations"][f]` lists the objects of the video whose `segmentations[f]` is non-empty, each with the reference's `ann_keys`
(`iscrowd`, `category_id` through the id map, `id`), `ori_id` where the annotation has one, `bbox` (XYWH) and `segmentation`.  A
`counts` list stays a list: the reference compresses it with `frPyObjects` only because pycocotools' decoder wants a string, and
`runs_from_rles` / `rle_decode` read both forms.  Polygons are not read: pycocotools' rasteriser is absent and cannot be pinned.
"""
import json
import os

from ..evaluation.vis_counts import runs_from_rles
from .datasets import _SOT_PREFIXES, _VIDEO_EXT, _record

_ANN_KEYS = ("iscrowd", "category_id", "id")                         # ytvis.py:220


def is_vos_name(dataset_name):
    """True for the names the reference registers with sot=True (builtin.py)."""
    return dataset_name.startswith(_SOT_PREFIXES)


def _category_id_map(data, dataset_name):
    """ytvis.py:156-191: category ids that are not 1 .. #categories are renumbered from 1 in the order of their values."""
    cat_ids = sorted(c["id"] for c in data.get("categories") or [])
    if not cat_ids or (min(cat_ids) == 1 and max(cat_ids) == len(cat_ids)):
        return None
    if "burst" in dataset_name:
        raise NotImplementedError(f"{dataset_name}: category ids outside 1 .. #categories go through the reference's BURST-to-LVIS table, "
                                  "which is not restated here")
    return {v: i + 1 for i, v in enumerate(cat_ids)}


def load_vos_json(json_file, image_root, dataset_name):
    """The records of a VOS test file in YouTube-VIS format, videos in the order of their ids, task "sot", `dataset_name` = "sot_" +
    the registered name.  A polygon segmentation is a NotImplementedError that names the video; a run-length code whose size is not
    the video's, or whose runs do not sum to H W, is the ValueError of `runs_from_rles`."""
    if not is_vos_name(dataset_name):
        raise ValueError(f"load_vos_json: {dataset_name!r} is no VOS data set (the names that begin with one of {_SOT_PREFIXES}); "
                         "data.load_video_json reads the others")
    with open(json_file) as f:
        data = json.load(f)
    id_map = _category_id_map(data, dataset_name)
    by_video = {}
    for anno in data.get("annotations") or []:
        by_video.setdefault(anno["video_id"], []).append(anno)
    records = []
    for vid in sorted(data["videos"], key=lambda v: v["id"]):
        names = [vid["file_names"]] if isinstance(vid["file_names"], str) else vid["file_names"]
        paths = [os.path.join(image_root, names[i]) for i in range(vid["length"])]
        if paths and os.path.dirname(paths[0]).rsplit(".", 1)[-1].lower() in _VIDEO_EXT:
            raise NotImplementedError(f"raw video input ({os.path.dirname(paths[0])}): torchvision.io is absent; convert the video to frames first")
        rec = _record(paths, vid["height"], vid["width"], vid["id"], "sot_" + dataset_name, "sot", has_mask=True)
        for key in ("framerate", "start_sec", "end_sec", "video"):
            if key in vid:
                rec[key] = vid[key]
        annos = by_video.get(vid["id"], [])
        codes = []
        for f in range(vid["length"]):
            for anno in annos:
                segms, boxes = anno.get("segmentations"), anno.get("bboxes")
                if not (segms and segms[f]):
                    continue
                segm = segms[f]
                if not isinstance(segm, dict):
                    raise NotImplementedError(f"video {vid['id']}: object {anno.get('id')} has a polygon segmentation in frame {f}; only "
                                              "run-length codes are read (pycocotools' rasteriser is absent)")
                obj = {key: anno[key] for key in _ANN_KEYS if key in anno}
                if "ori_id" in anno:
                    obj["ori_id"] = anno["ori_id"]
                obj["bbox"] = boxes[f] if boxes else None
                obj["segmentation"] = segm
                if id_map:
                    obj["category_id"] = id_map[obj["category_id"]]
                rec["annotations"][f].append(obj)
                codes.append(segm)
        runs_from_rles(codes, vid["height"], vid["width"], video=vid["id"])    # (the check of every code, once, where the file is read)
        records.append(rec)
    return records
