"""The records the test mapper reads: `load_ytvis_json` (univs/data/datasets/ytvis.py:143-375) for test files, without detectron2's
catalog and the YTVOS api, and the folder walk of datasets/data_utils/custom_videos/convert_custom_videos_to_coco_test.py:61-78.

Test mode only: the per-frame annotation lists of a record are empty.  The reference fills them from `segmentations` / `bboxes`, and its
test mapper reads them only for task "sot" (first-frame masks): those records come from vos_datasets.py."""
import json
import os

from .images import read_image

# builtin.py:493-497; the reference marks their records `is_raw_video` and its mapper clears the mark again for a path that is no
# video file (dataset_mapper_uni_vid.py:328-331).  Raw video files are not read here, so the mark is never set.
CUSTOM_NAMES = ("custom_images", "custom_videos", "custom_videos_text", "custom_videos_text_internvid")
# ytvis.py:353-367, for the data sets the drivers serve
_DETECTION_PREFIXES = (("ytvis_2019", "ytvis19"), ("ytvis_2021", "ytvis21"), ("ovis", "ovis"), ("vipseg", "vipseg"), ("vspw", "vspw"))
_VIDEO_EXT = ("mp4", "avi", "mov", "mkv")
_SOT_PREFIXES = ("sot_", "mots_mose", "mots_burst", "pvos_")          # builtin.py: the splits registered with sot=True


def task_and_name(dataset_name):
    """(task, the record's dataset_name) of a registered name, ytvis.py:329-377."""
    if dataset_name.startswith("rvos"):                              # builtin.py:421-442: registered with has_expression=True
        return "grounding", dataset_name
    if dataset_name.startswith(_SOT_PREFIXES) or "sa_1b" in dataset_name:
        if dataset_name.startswith(_SOT_PREFIXES):
            raise NotImplementedError(f"task \"sot\" ({dataset_name}): data.load_vos_json (vos_datasets.py) reads the VOS data sets, with their "
                                      "first-frame masks, and data.VOSTestMapper maps them")
        raise NotImplementedError(f"task \"sot\" ({dataset_name}): SA-1B stores polygons, and no polygon rasteriser is built here")
    for prefix, name in _DETECTION_PREFIXES:
        if dataset_name.startswith(prefix):
            return "detection", name
    if dataset_name in CUSTOM_NAMES:
        return "detection", dataset_name
    raise ValueError(f"Unsupported dataset_name: {dataset_name} ")


def _record(file_names, height, width, video_id, dataset_name, task, has_mask):
    return {"file_names": list(file_names), "height": int(height), "width": int(width), "length": len(file_names), "video_id": video_id,
            "annotations": [[] for _ in file_names], "has_mask": has_mask, "has_caption": False, "has_stuff": False,
            "is_raw_video": False, "task": task, "dataset_name": dataset_name}


def load_video_json(json_file, image_root, dataset_name):
    """The records of a YouTube-VIS-format test file, videos in the order of their ids.  Expression files (the "rvos*" names) add
    `exp_id` / `expressions`, one entry per annotation of the video."""
    task, name = task_and_name(dataset_name)
    with open(json_file) as f:
        data = json.load(f)
    by_video = {}
    for anno in data.get("annotations") or []:
        by_video.setdefault(anno["video_id"], []).append(anno)
    records = []
    for vid in sorted(data["videos"], key=lambda v: v["id"]):
        names = [vid["file_names"]] if isinstance(vid["file_names"], str) else vid["file_names"]
        paths = [os.path.join(image_root, names[i]) for i in range(vid["length"])]
        # dataset_mapper_uni_vid.py:329-330: frames named inside a video file stand for that file's frames
        if paths and os.path.dirname(paths[0]).rsplit(".", 1)[-1].lower() in _VIDEO_EXT:
            raise NotImplementedError(f"raw video input ({os.path.dirname(paths[0])}): torchvision.io is absent; convert the video to frames first")
        rec = _record(paths, vid["height"], vid["width"], vid["id"], name, task, has_mask=dataset_name not in CUSTOM_NAMES)
        for key in ("framerate", "start_sec", "end_sec", "video"):
            if key in vid:
                rec[key] = vid[key]
        if task == "grounding":
            annos = by_video.get(vid["id"], [])
            for anno in annos:
                assert "expressions" in anno and "exp_id" in anno, f"{json_file}: an annotation of video {vid['id']} has no expression"
            rec["exp_id"] = [anno["exp_id"] for anno in annos]
            rec["expressions"] = [anno["expressions"] for anno in annos]
        records.append(rec)
    return records


def video_records_from_dir(video_dir, dataset_name="custom_videos"):
    """One record per sub-folder of `video_dir` that holds frames: its jpg / png files sorted by name, the size read from the first
    one, the folder's name as the video id.  Files that are not folders are raw videos, which are not read here."""
    task, name = task_and_name(dataset_name)
    records = []
    for video_name in sorted(os.listdir(video_dir)):
        path = os.path.join(video_dir, video_name)
        if not os.path.isdir(path):
            if video_name.rsplit(".", 1)[-1].lower() in _VIDEO_EXT:
                raise NotImplementedError(f"raw video input ({path}): torchvision.io is absent; convert the video to frames first")
            continue
        frames = sorted(n for n in os.listdir(path) if n.split(".")[-1] in ("jpg", "png"))
        if not frames:
            continue
        height, width = read_image(os.path.join(path, frames[0])).shape[:2]      # (oriented by its EXIF tag, as the mapper will read it)
        records.append(_record([os.path.join(path, n) for n in frames], height, width, video_name, name, task, has_mask=False))
    return records
