"""The records the image test mapper reads: a folder of images, or a panoptic annotation file in COCO's format -- the reference's
`load_coco_panoptic_json` / `load_ade20k_panoptic_json` (univs/data/datasets/coco_panoptic.py:232-284, ade20k_panoptic.py:194-244)
without detectron2's catalog.  The class table comes from the file's own `categories`: no category list is kept in this repository."""
import json
import os

_IMAGE_EXT = ("jpg", "png")


def image_records_from_dir(folder):
    """One record {"file_name", "image_id"} per jpg / png file of `folder`, sorted by name; the image id is the file's stem."""
    names = sorted(n for n in os.listdir(folder) if n.split(".")[-1] in _IMAGE_EXT and os.path.isfile(os.path.join(folder, n)))
    return [{"file_name": os.path.join(folder, n), "image_id": os.path.splitext(n)[0]} for n in names]


def class_table(categories):
    """The class table of a panoptic json's `categories` list: {"ids": [dataset id per contiguous index = position in the file],
    "names", "isthing", "colors" (None where the file has none), "dataset_id_to_contiguous_id", "thing_contiguous_ids"}."""
    ids = [int(c["id"]) for c in categories]
    if len(set(ids)) != len(ids):
        raise ValueError("categories: a dataset id occurs twice")
    isthing = [bool(c.get("isthing", 1)) for c in categories]
    return {"ids": ids, "names": [str(c.get("name", c["id"])) for c in categories], "isthing": isthing,
            "colors": [c.get("color") for c in categories],
            "dataset_id_to_contiguous_id": {d: i for i, d in enumerate(ids)},
            "thing_contiguous_ids": [i for i, t in enumerate(isthing) if t]}


def load_categories_json(json_file):
    """`class_table` of a file that holds a `categories` list (a panoptic json, or one written for --categories-json)."""
    with open(json_file) as f:
        return class_table(json.load(f)["categories"])


def load_panoptic_json(json_file, image_dir, gt_dir, semseg_dir=None):
    """(records, class table).  One record per annotation of the file, in its order: "file_name" (the annotation's file name with the
    extension ".jpg", under `image_dir`), "image_id", "pan_seg_file_name" (under `gt_dir`), "sem_seg_file_name" (under `semseg_dir`,
    when given) and "segments_info" with `category_id` mapped to the contiguous index and `isthing` set from the class table -- the
    reference's `_convert_category_id`.  The image id is kept as the file has it (COCO's reference loader makes it an int, ADE20K's
    keeps the string).  As the reference, the first record's files must exist."""
    with open(json_file) as f:
        info = json.load(f)
    table = class_table(info["categories"])
    to_contiguous = table["dataset_id_to_contiguous_id"]
    records = []
    for ann in info["annotations"]:
        segments = []
        for seg in ann["segments_info"]:
            seg = dict(seg)
            c = to_contiguous[int(seg["category_id"])]
            seg["category_id"], seg["isthing"] = c, table["isthing"][c]
            segments.append(seg)
        rec = {"file_name": os.path.join(image_dir, os.path.splitext(ann["file_name"])[0] + ".jpg"), "image_id": ann["image_id"],
               "pan_seg_file_name": os.path.join(gt_dir, ann["file_name"]), "segments_info": segments}
        if semseg_dir is not None:
            rec["sem_seg_file_name"] = os.path.join(semseg_dir, ann["file_name"])
        records.append(rec)
    assert len(records), f"No images found in {image_dir}!"
    for key in ("file_name", "pan_seg_file_name", "sem_seg_file_name"):
        assert key not in records[0] or os.path.isfile(records[0][key]), records[0][key]
    return records, table
