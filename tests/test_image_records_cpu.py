"""CPU: images from disk to the per-image driver (data/image_datasets.py, data/image_mapper.py, engine.inference_on_images): the
records and the class table of a synthetic panoptic json, the records of a folder, the mapper's dictionary against `VideoTestMapper`'s
tensors for the same file and config, and the loop's batching and merging."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.frames_cases import frames
from univs_amd.config import get_cfg
from univs_amd.data import (ImageTestMapper, VideoTestMapper, class_table, image_records_from_dir, load_categories_json, load_panoptic_json,
                            resize_params_from_config)
from univs_amd.engine import inference_on_images

H, W = 37, 53
CATEGORIES = [{"id": 1, "name": "person", "isthing": 1}, {"id": 17, "name": "sky", "isthing": 0}, {"id": 3, "name": "car", "isthing": 1},
              {"id": 200, "name": "road", "isthing": 0}]            # two things, two stuff classes, out of id order


def write_tree(root):
    """Three images val/<name>.jpg, pan/<name>.png, sem/<name>.png and the json; one crowd segment."""
    for sub in ("val", "pan", "sem"):
        os.makedirs(os.path.join(root, sub))
    src = frames("noise", 3, H, W)
    names = ["000000000139", "000000000285", "000000000632"]
    annotations = []
    for k, name in enumerate(names):
        Image.fromarray(src[k]).save(os.path.join(root, "val", name + ".jpg"))
        Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(os.path.join(root, "pan", name + ".png"))
        Image.fromarray(np.zeros((H, W), np.uint8)).save(os.path.join(root, "sem", name + ".png"))
        segs = [{"id": 10 + k, "category_id": 17, "iscrowd": 0, "area": 100, "bbox": [0, 0, 10, 10]},
                {"id": 20 + k, "category_id": 1, "iscrowd": int(k == 1), "area": 50, "bbox": [5, 5, 10, 5]},
                {"id": 30 + k, "category_id": 200, "iscrowd": 0, "area": 7, "bbox": [1, 2, 3, 4]}]
        annotations.append({"image_id": int(name), "file_name": name + ".png", "segments_info": segs})
    path = os.path.join(root, "panoptic_val.json")
    with open(path, "w") as f:
        json.dump({"images": [{"id": int(n), "file_name": n + ".jpg", "height": H, "width": W} for n in names], "annotations": annotations,
                   "categories": CATEGORIES}, f)
    return path, names, src


def test_class_table_is_read_from_the_files_own_categories(tmp_path):
    path, _, _ = write_tree(str(tmp_path))
    t = load_categories_json(path)
    assert t == class_table(CATEGORIES)
    assert t["ids"] == [1, 17, 3, 200] and t["names"] == ["person", "sky", "car", "road"] and t["isthing"] == [True, False, True, False]
    assert t["dataset_id_to_contiguous_id"] == {1: 0, 17: 1, 3: 2, 200: 3} and t["thing_contiguous_ids"] == [0, 2]
    with pytest.raises(ValueError):
        class_table(CATEGORIES + [{"id": 3, "name": "again", "isthing": 1}])


def test_records_of_a_panoptic_json(tmp_path):
    path, names, _ = write_tree(str(tmp_path))
    val, pan, sem = (os.path.join(str(tmp_path), s) for s in ("val", "pan", "sem"))
    records, table = load_panoptic_json(path, val, pan, sem)
    assert table == class_table(CATEGORIES) and len(records) == 3
    for k, (r, name) in enumerate(zip(records, names)):
        assert r["file_name"] == os.path.join(val, name + ".jpg") and r["image_id"] == int(name)
        assert r["pan_seg_file_name"] == os.path.join(pan, name + ".png") and r["sem_seg_file_name"] == os.path.join(sem, name + ".png")
        assert sorted(r) == ["file_name", "image_id", "pan_seg_file_name", "segments_info", "sem_seg_file_name"]
        assert [(s["id"], s["category_id"], s["isthing"], s["iscrowd"]) for s in r["segments_info"]] == \
            [(10 + k, 1, False, 0), (20 + k, 0, True, int(k == 1)), (30 + k, 3, False, 0)]
        assert r["segments_info"][0]["area"] == 100 and r["segments_info"][2]["bbox"] == [1, 2, 3, 4]
    assert sum(s["iscrowd"] for r in records for s in r["segments_info"]) == 1
    without, _ = load_panoptic_json(path, val, pan)
    assert all("sem_seg_file_name" not in r for r in without)
    assert json.load(open(path))["annotations"][0]["segments_info"][0]["category_id"] == 17       # the file's own dicts are not touched
    with pytest.raises(AssertionError):
        load_panoptic_json(path, os.path.join(str(tmp_path), "nowhere"), pan)
    with pytest.raises(KeyError):                                    # a segment of a category the file does not list
        bad = json.load(open(path))
        bad["annotations"][0]["segments_info"][0]["category_id"] = 99
        json.dump(bad, open(os.path.join(str(tmp_path), "bad.json"), "w"))
        load_panoptic_json(os.path.join(str(tmp_path), "bad.json"), val, pan)


def test_records_of_a_folder_are_sorted(tmp_path):
    src = frames("noise", 3, H, W)
    for k, name in enumerate(("b.jpg", "c.png", "a.jpg")):
        Image.fromarray(src[k]).save(tmp_path / name)
    (tmp_path / "notes.txt").write_text("no image")
    os.makedirs(tmp_path / "d.jpg")                                  # a folder is no image
    records = image_records_from_dir(str(tmp_path))
    assert records == [{"file_name": str(tmp_path / n), "image_id": n[:-4]} for n in ("a.jpg", "b.jpg", "c.png")]


def image_cfg(n=1, fmt="RGB"):
    cfg = get_cfg()
    cfg.INPUT.SAMPLING_FRAME_NUM = n
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST = 20, 40
    cfg.INPUT.LSJ_AUG.IMAGE_SIZE = 26                                # the LSJ square caps the long edge
    cfg.INPUT.FORMAT = fmt
    return cfg


@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
def test_mapper_tensors_equal_the_video_mappers(tmp_path, fmt):
    path, names, _ = write_tree(str(tmp_path))
    val, pan = os.path.join(str(tmp_path), "val"), os.path.join(str(tmp_path), "pan")
    records, _ = load_panoptic_json(path, val, pan)
    cfg = image_cfg(2, fmt)
    assert resize_params_from_config(cfg) == (20, 26)
    mapper = ImageTestMapper.from_config(cfg, resize="host")
    d = mapper(records[1])
    video = VideoTestMapper.from_config(cfg, resize="host")._host([records[1]["file_name"]])[0]
    assert len(d["image"]) == len(d["image_padding_mask"]) == 2
    for im, pad in zip(d["image"], d["image_padding_mask"]):
        assert im.dtype == torch.uint8 and tuple(im.shape) == (3, 18, 26) and torch.equal(im, video)
        assert pad.dtype == torch.uint8 and tuple(pad.shape) == (18, 26) and not pad.any()
    assert d["file_names"] == [records[1]["file_name"]] * 2 and d["file_name"] == records[1]["file_name"]
    assert (d["height"], d["width"]) == (H, W) and d["task"] == "detection" and d["dataset_name"] == "coco_panoptic" and d["has_stuff"] is True
    assert d["video_len"] == 2 and d["frame_indices"] == [0, 1] and d["instances"] == [] and d["image_id"] == int(names[1])
    assert "file_name" in records[1] and "image" not in records[1]  # the record is left as it was
    # a folder record: no panoptic file, so "coco"; a name the record carries is kept
    plain = mapper({"file_name": records[0]["file_name"], "image_id": "x"})
    assert plain["dataset_name"] == "coco" and plain["has_stuff"] is False and "file_name" not in plain
    assert mapper({"file_name": records[0]["file_name"], "image_id": "x", "dataset_name": "ade20k"})["dataset_name"] == "ade20k"


def test_mapper_refuses_training_and_bad_switches():
    with pytest.raises(NotImplementedError, match="training"):
        ImageTestMapper.from_config(image_cfg(), is_train=True)
    with pytest.raises(ValueError):
        ImageTestMapper(20, 40, resize="tpu")
    with pytest.raises(ValueError):
        ImageTestMapper(20, 40, decode="gpu", resize="host")


class Recorder:
    def __init__(self, key):
        self.key, self.calls = key, []

    def reset(self):
        self.calls = ["reset"]

    def process(self, inputs, outputs):
        self.calls.append(([i["n"] for i in inputs], list(outputs)))

    def evaluate(self):
        return {self.key: {"seen": sum(len(c[0]) for c in self.calls[1:])}}


def test_the_loop_batches_and_merges():
    records = [{"n": k} for k in range(5)]
    sizes = []

    def model(inputs):
        sizes.append(len(inputs))
        return [10 * i["n"] for i in inputs]
    a, b = Recorder("a"), Recorder("b")
    seen = []
    out = inference_on_images(model, records, dict, [a, b], on_output=lambda i, o: seen.append(o), batch=2)
    assert sizes == [2, 2, 1] and out == {"a": {"seen": 5}, "b": {"seen": 5}}
    assert a.calls == ["reset", ([0, 1], [0, 10]), ([2, 3], [20, 30]), ([4], [40])] == b.calls and seen == [[0, 10], [20, 30], [40]]
    assert inference_on_images(model, records, dict, batch=1) == [0, 10, 20, 30, 40]
    assert inference_on_images(model, records, dict, a) == {"a": {"seen": 5}}
    with pytest.raises(AssertionError, match="same key"):
        inference_on_images(model, records, dict, [Recorder("k"), Recorder("k")])
