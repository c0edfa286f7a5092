"""CPU: frames from disk to the drivers (univs_amd/data, univs_amd/engine.py) with resize="host": a temporary folder of small PNGs ->
records -> the mapper's dictionary; BGR; a grounding record; what is not built says so; the inference loop's order of calls."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.frames_cases import frames
from univs_amd.config import get_cfg
from univs_amd.data import VideoTestMapper, load_video_json, read_image, resize_params_from_config, video_records_from_dir
from univs_amd.data.resize_rule import resize_u8_reference, shortest_edge_size
from univs_amd.engine import inference_on_videos

H, W, N = 37, 53, 3


def write_videos(root, names=("b_video", "a_video"), n=N, h=H, w=W):
    """<root>/<name>/<frame>.png, frame names written out of order; returns {name: uint8 [n, h, w, 3]} in frame order."""
    out = {}
    for k, name in enumerate(names):
        os.makedirs(os.path.join(root, name))
        src = frames("noise", n, h + k, w)
        for i in reversed(range(n)):
            Image.fromarray(src[i]).save(os.path.join(root, name, f"{i:05d}.png"))
        with open(os.path.join(root, name, "notes.txt"), "w") as f:
            f.write("not a frame")
        out[name] = src
    return out


def test_records_from_a_folder_of_frames(tmp_path):
    write_videos(str(tmp_path))
    records = video_records_from_dir(str(tmp_path))
    assert [r["video_id"] for r in records] == ["a_video", "b_video"]
    r = records[0]
    assert (r["height"], r["width"], r["length"]) == (H + 1, W, N)
    assert [os.path.basename(p) for p in r["file_names"]] == [f"{i:05d}.png" for i in range(N)]
    assert r["task"] == "detection" and r["dataset_name"] == "custom_videos" and r["is_raw_video"] is False
    assert r["has_mask"] is False and r["has_caption"] is False and r["annotations"] == [[]] * N


def test_host_mapper_keys_dtypes_sizes_and_order(tmp_path):
    src = write_videos(str(tmp_path))
    records = video_records_from_dir(str(tmp_path))
    mapper = VideoTestMapper(20, 26, resize="host")
    d = mapper(records[1])
    newh, neww = shortest_edge_size(H, W, 20, 26)
    assert (newh, neww) == (18, 26)                                  # the long side meets max_size
    assert d["video_id"] == "b_video" and d["video_len"] == N and d["frame_indices"] == [0, 1, 2] and d["instances"] == []
    assert (d["height"], d["width"]) == (H, W)                       # the original size
    assert d["file_names"] == records[1]["file_names"] and "annotations" not in d
    assert len(d["image"]) == len(d["image_padding_mask"]) == N
    for i, (im, pad) in enumerate(zip(d["image"], d["image_padding_mask"])):
        assert im.dtype == torch.uint8 and tuple(im.shape) == (3, newh, neww) and im.device.type == "cpu" and im.is_contiguous()
        assert pad.dtype == torch.uint8 and tuple(pad.shape) == (newh, neww) and not pad.any()
        assert np.array_equal(im.numpy(), resize_u8_reference(src["b_video"][i], newh, neww).transpose(2, 0, 1)), i
    assert records[1]["file_names"] and "image" not in records[1]    # the record is left as it was


def test_bgr_reverses_the_channels(tmp_path):
    write_videos(str(tmp_path), names=("v",))
    rec = video_records_from_dir(str(tmp_path))[0]
    rgb = VideoTestMapper(20, 100, "RGB")(rec)["image"]
    bgr = VideoTestMapper(20, 100, "BGR")(rec)["image"]
    assert all(torch.equal(a.flip(0), b) for a, b in zip(rgb, bgr))
    path = rec["file_names"][0]
    assert np.array_equal(read_image(path, "BGR"), read_image(path, "RGB")[:, :, ::-1])
    with pytest.raises(ValueError, match="format"):
        read_image(path, "L")


def test_read_image_applies_the_exif_orientation(tmp_path):
    a = frames("noise", 1, 6, 9)[0]
    exif = Image.Exif()
    exif[274] = 6                                                    # stored rotated: the viewer turns it by 270 degrees
    Image.fromarray(a).save(tmp_path / "r.png", exif=exif)
    got = read_image(str(tmp_path / "r.png"))
    assert got.shape == (9, 6, 3) and np.array_equal(got, np.asarray(Image.fromarray(a).transpose(Image.ROTATE_270)))


def test_from_config_follows_the_test_branch_of_build_augmentation():
    cfg = get_cfg()
    cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, cfg.INPUT.FORMAT = 720, 1280, "BGR"
    cfg.INPUT.LSJ_AUG.SQUARE_ENABLED, cfg.INPUT.LSJ_AUG.IMAGE_SIZE = True, 1024
    assert resize_params_from_config(cfg) == (720, 1024)
    cfg.INPUT.LSJ_AUG.SQUARE_ENABLED = False
    assert resize_params_from_config(cfg) == (720, 1280)
    m = VideoTestMapper.from_config(cfg)
    assert (m.short, m.max_size, m.image_format, m.resize) == (720, 1280, "BGR", "host")


def video_json(tmp_path, annotations=None, names=None):
    src = write_videos(str(tmp_path / "JPEGImages"), names=("v1", "v0"))
    videos = [{"id": 7, "file_names": [f"v1/{i:05d}.png" for i in range(N)], "height": H, "width": W, "length": N},
              {"id": 3, "file_names": [f"v0/{i:05d}.png" for i in range(N)], "height": H + 1, "width": W, "length": N}]
    data = {"videos": videos, "categories": [{"id": 1, "name": "object"}]}
    if annotations is not None:
        data["annotations"] = annotations
    path = tmp_path / "test.json"
    path.write_text(json.dumps(data))
    return str(path), str(tmp_path / "JPEGImages"), src


@pytest.mark.parametrize("registered,name", [("ytvis_2019_val", "ytvis19"), ("ytvis_2021_val", "ytvis21"), ("ovis_val", "ovis"),
                                             ("vipseg_panoptic_val", "vipseg"), ("vspw_vss_video_val", "vspw"),
                                             ("custom_videos_text", "custom_videos_text")])
def test_records_of_a_test_json(tmp_path, registered, name):
    path, root, _ = video_json(tmp_path)
    records = load_video_json(path, root, registered)
    assert [r["video_id"] for r in records] == [3, 7]               # in the order of the ids
    r = records[1]
    assert r["file_names"] == [os.path.join(root, f"v1/{i:05d}.png") for i in range(N)]
    assert (r["height"], r["width"], r["length"], r["dataset_name"], r["task"]) == (H, W, N, name, "detection")
    assert r["has_mask"] is (not registered.startswith("custom")) and r["has_caption"] is False and r["is_raw_video"] is False
    assert r["annotations"] == [[]] * N and "expressions" not in r
    with pytest.raises(ValueError, match="Unsupported dataset_name"):
        load_video_json(path, root, "kitti_step_val")


def test_grounding_record_and_its_expressions(tmp_path):
    annos = [{"video_id": 7, "id": 1, "exp_id": 0, "expressions": ["A large_dog (2) on the left."]},
             {"video_id": 7, "id": 2, "exp_id": 1, "expressions": ["the person's red-hat"]},
             {"video_id": 3, "id": 3, "exp_id": 0, "expressions": [["a cat", "The CAT, sleeping"]]}]
    path, root, _ = video_json(tmp_path, annos)
    records = load_video_json(path, root, "rvos-refytb-val")
    r = records[1]
    assert r["task"] == "grounding" and r["dataset_name"] == "rvos-refytb-val" and r["exp_id"] == [0, 1]
    assert r["expressions"] == [["A large_dog (2) on the left."], ["the person's red-hat"]]
    d = VideoTestMapper(20, 100)(r)
    assert d["expressions"] == ["a large dog  on the left", "the persons red hat"] and d["exp_obj_ids"] == [0, 1]
    assert len(d["image"]) == N and "mask_palette" not in d
    d = VideoTestMapper(20, 100)(records[0])                         # the ref-davis form: a list of several expressions per object
    assert d["expressions"] == [["a cat", "the cat sleeping"]] and d["exp_obj_ids"] == [0]
    assert records[0]["expressions"] == [[["a cat", "The CAT, sleeping"]]]           # the record is not cleaned in place


def test_ref_davis_record_carries_the_annotation_palette(tmp_path):
    annos = [{"video_id": 7, "id": 1, "exp_id": 0, "expressions": [["a dog"]]}, {"video_id": 3, "id": 1, "exp_id": 0, "expressions": [["a cat"]]}]
    path, root, _ = video_json(tmp_path, annos)
    os.makedirs(tmp_path / "Annotations" / "v1")
    im = Image.fromarray(np.zeros((H, W), np.uint8), mode="P")
    im.putpalette([0, 0, 0, 128, 0, 0, 0, 128, 0] + [0] * 759)
    im.save(tmp_path / "Annotations" / "v1" / "00000.png")
    records = load_video_json(path, root, "rvos-refdavis-val-0")
    d = VideoTestMapper(20, 100)(records[1])                         # video 7 = v1: its first annotation PNG's palette
    assert d["mask_palette"][:9] == [0, 0, 0, 128, 0, 0, 0, 128, 0] and d["expressions"] == [["a dog"]]
    assert VideoTestMapper(20, 100)(records[0])["mask_palette"] is None               # v0 has no annotation folder


def test_what_is_not_built_says_so(tmp_path):
    path, root, _ = video_json(tmp_path)
    with pytest.raises(NotImplementedError, match="sot"):
        load_video_json(path, root, "sot_davis17_val")
    rec = load_video_json(path, root, "ovis_val")[0]
    with pytest.raises(NotImplementedError, match="sot"):
        VideoTestMapper(20, 100)(dict(rec, task="sot"))
    with pytest.raises(NotImplementedError, match="raw video"):
        VideoTestMapper(20, 100)(dict(rec, is_raw_video=True))
    (tmp_path / "raw").mkdir()
    (tmp_path / "raw" / "clip.mp4").write_bytes(b"")
    with pytest.raises(NotImplementedError, match="raw video"):
        video_records_from_dir(str(tmp_path / "raw"))
    raw = {"videos": [{"id": "clip", "file_names": [f"clip.mp4/{i:06d}.jpg" for i in range(N)], "height": H, "width": W, "length": N}]}
    (tmp_path / "raw.json").write_text(json.dumps(raw))             # frames named inside a video file: the reference decodes the file
    with pytest.raises(NotImplementedError, match="raw video"):
        load_video_json(str(tmp_path / "raw.json"), root, "custom_videos")
    with pytest.raises(NotImplementedError, match="training"):
        VideoTestMapper(20, 100, is_train=True)
    with pytest.raises(ValueError, match="resize"):
        VideoTestMapper(20, 100, resize="device")


def test_inference_loop_calls_mapper_model_and_evaluator_in_order(tmp_path):
    write_videos(str(tmp_path))
    records = video_records_from_dir(str(tmp_path))
    log = []

    class Evaluator:
        def reset(self):
            log.append("reset")

        def process(self, inputs, outputs):
            assert len(inputs) == 1 and outputs == {"n": len(inputs[0]["image"]), "id": inputs[0]["video_id"]}
            log.append(("process", inputs[0]["video_id"]))

        def evaluate(self):
            log.append("evaluate")
            return {"score": 1.0}

    def model(inputs):
        assert not torch.is_grad_enabled()
        log.append(("model", inputs[0]["video_id"]))
        return {"n": len(inputs[0]["image"]), "id": inputs[0]["video_id"]}

    mapper = VideoTestMapper(20, 100)
    assert inference_on_videos(model, records, mapper, Evaluator()) == {"score": 1.0}
    assert log == ["reset", ("model", "a_video"), ("process", "a_video"), ("model", "b_video"), ("process", "b_video"), "evaluate"]
    assert inference_on_videos(model, records, mapper) == [{"n": N, "id": "a_video"}, {"n": N, "id": "b_video"}]


def test_command_line_arguments():
    from univs_amd import run
    a = run.parse_args(["--config-file", "c.yaml", "--weights", "w.pth", "--video-dir", "d", "--output-dir", "o", "INPUT.MIN_SIZE_TEST", "512"])
    assert (a.resize, a.video_dir, a.opts) == ("gpu", "d", ["INPUT.MIN_SIZE_TEST", "512"]) and run.build_evaluator(a) is None
    for bad in (["--json", "j"], ["--json", "j", "--image-root", "r", "--dataset-name", "n", "--video-dir", "d"], [],
                ["--video-dir", "d", "--pan-gt-json", "p"]):
        with pytest.raises(SystemExit):
            run.parse_args(["--config-file", "c", "--weights", "w", "--output-dir", "o"] + bad)
