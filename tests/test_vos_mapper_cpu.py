"""CPU: VOS from disk (univs_amd/data/vos_datasets.py, vos_mapper.py) with resize="host": a json and frames written into a temporary
folder -> records -> the mapper's per-frame annotations, against a pipeline written out here (rle_decode -> Pillow NEAREST -> boxes
from `any`); what is not read says so; the VOS driver places the mapper's masks; the command line's VOS arguments."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from tests import prompt_masks_cases as pc
from univs_amd.data import VideoTestMapper, VOSTestMapper, is_vos_name, load_video_json, load_vos_json, shortest_edge_size
from univs_amd.inference.results import rle_decode
from univs_amd.inference.video_vos import FrameAnnotations

H, W, N = pc.VOS_H, pc.VOS_W, pc.VOS_N
SHORT, MAX = 20, 100


@pytest.fixture
def dataset(tmp_path):
    return pc.write_vos_dataset(str(tmp_path))


def test_names():
    assert all(is_vos_name(n) for n in ("sot_davis17_val", "sot_ytbvos18_val", "mots_mose_val", "mots_burst_val", "pvos_viposeg_val"))
    assert not any(is_vos_name(n) for n in ("ytvis_2021_val", "rvos-refytb-val", "custom_videos", "mots_bdd_seg_track_val"))


def test_records(dataset):
    path, root, truth = dataset
    records = load_vos_json(path, root, "sot_davis17_val")
    assert [r["video_id"] for r in records] == [2, 5]               # in the order of the ids
    r = records[1]
    assert (r["task"], r["dataset_name"], r["height"], r["width"], r["length"]) == ("sot", "sot_sot_davis17_val", H, W, N)
    assert r["file_names"] == [os.path.join(root, f"a/{i:05d}.png") for i in range(N)]
    assert r["has_mask"] is True and r["is_raw_video"] is False
    assert [[o["id"] for o in objs] for objs in r["annotations"]] == [[1, 2, 9], [], [2, 3], []]
    first = r["annotations"][0]
    # the category ids 3 and 7 are not 1 .. 2: renumbered from 1 in their order
    assert first[0] == {"iscrowd": 0, "category_id": 2, "id": 1, "ori_id": 41, "bbox": [1, 2, 3, 4],
                        "segmentation": pc.code_of(truth[5, 0][1])}
    assert isinstance(first[0]["segmentation"]["counts"], list)      # a list of counts stays a list
    assert "ori_id" not in first[1] and first[1]["category_id"] == 1 and isinstance(first[1]["segmentation"]["counts"], str)
    assert first[2]["iscrowd"] == 1
    assert [[o["id"] for o in objs] for objs in records[0]["annotations"]] == [[4], [], [], []] and records[0]["height"] == H + 1
    with pytest.raises(ValueError, match="no VOS data set"):
        load_vos_json(path, root, "ytvis_2021_val")


def reference_frame(objs, out_hw):
    """The pipeline of the reference's mapper for one frame, written out: (masks bool [n, h, w], boxes float32 [n, 4])."""
    planes = []
    for o in objs:
        code = o["segmentation"]
        if isinstance(code["counts"], list):                        # (what `frPyObjects` + `decode` give for a list of counts)
            flat = np.repeat(np.arange(len(code["counts"])) % 2, code["counts"]).astype(np.uint8)
            plane = flat.reshape(code["size"][1], code["size"][0]).T
        else:
            plane = rle_decode(code)
        planes.append(pc.pillow_resize(plane, out_hw))
    masks = np.stack(planes)
    return torch.from_numpy(masks).bool(), torch.from_numpy(pc.any_boxes(masks)).float()


def check_mapped(d, record, truth):
    out_hw = shortest_edge_size(record["height"], record["width"], SHORT, MAX)
    assert len(d["instances"]) == len(d["image"]) == record["length"] and "annotations" not in d
    for f, (ann, objs) in enumerate(zip(d["instances"], record["annotations"])):
        assert isinstance(ann, FrameAnnotations) and ann.image_size == out_hw == tuple(d["image"][f].shape[1:])
        objs = [o for o in objs if o["iscrowd"] == 0]
        assert len(ann) == len(objs)
        if not objs:
            assert ann.ori_ids == [] and tuple(ann.gt_masks.shape) == (0,) + out_hw and tuple(ann.gt_boxes.tensor.shape) == (0, 4)
            continue
        masks, boxes = reference_frame(objs, out_hw)
        assert ann.gt_masks.dtype == torch.bool and torch.equal(ann.gt_masks.cpu(), masks)
        assert ann.gt_boxes.tensor.dtype == torch.float32 and torch.equal(ann.gt_boxes.tensor.cpu(), boxes)
        assert ann.gt_classes.dtype == torch.int64 and ann.gt_classes.tolist() == [o["category_id"] for o in objs]
        assert ann.ori_ids == [o.get("ori_id", o["id"]) for o in objs]
        for o, m in zip(objs, masks):                               # ... and the decoded codes are the masks that were written
            assert np.array_equal(m.numpy(), pc.pillow_resize(truth[record["video_id"], f][o["id"]], out_hw))


def test_host_mapper_against_the_written_out_pipeline(dataset):
    path, root, truth = dataset
    records = load_vos_json(path, root, "sot_davis17_val")
    before = copy.deepcopy(records)
    mapper = VOSTestMapper(SHORT, MAX, resize="host")
    for record in records:
        d = mapper(record)
        check_mapped(d, record, truth)
        assert d["task"] == "sot" and d["video_len"] == N and (d["height"], d["width"]) == (record["height"], record["width"])
    assert records == before                                        # the records are left as they were
    d = mapper(records[1])
    assert [a.ori_ids for a in d["instances"]] == [[41, 2], [], [2, 43], []]      # the crowd object is dropped
    assert [a.gt_classes.tolist() for a in d["instances"]] == [[2, 1], [], [1, 2], []]
    assert d["mask_palette"][:9] == [0, 0, 0, 128, 0, 0, 0, 128, 0] and mapper(records[0])["mask_palette"] is None
    plain = VideoTestMapper(SHORT, MAX)(dict(records[1], task="detection"))
    assert all(torch.equal(a, b) for a, b in zip(d["image"], plain["image"]))      # frames exactly as in the parent
    with pytest.raises(ValueError, match="task"):
        mapper(dict(records[1], task="detection"))


def test_the_old_entry_points_still_refuse_and_name_the_new_ones(dataset):
    path, root, _ = dataset
    with pytest.raises(NotImplementedError, match="load_vos_json"):
        load_video_json(path, root, "sot_davis17_val")
    rec = load_vos_json(path, root, "sot_davis17_val")[0]
    with pytest.raises(NotImplementedError, match="VOSTestMapper"):
        VideoTestMapper(SHORT, MAX)(rec)


def test_polygons_and_wrong_sizes_raise(dataset, tmp_path):
    path, root, _ = dataset
    data = json.load(open(path))

    def variant(change):
        bad = copy.deepcopy(data)
        change(bad["annotations"][0]["segmentations"])
        p = tmp_path / "bad.json"
        p.write_text(json.dumps(bad))
        return str(p)

    def polygon(segms):
        segms[0] = [[1.0, 1.0, 9.0, 1.0, 9.0, 9.0]]

    def other_size(segms):
        segms[0] = pc.code_of(pc.mask("blob", H + 1, W))

    def short_runs(segms):
        segms[0] = {"size": [H, W], "counts": [5, 7, H * W - 13]}

    with pytest.raises(NotImplementedError, match="video 5.*polygon"):
        load_vos_json(variant(polygon), root, "sot_davis17_val")
    with pytest.raises(ValueError, match="video 5.*size"):
        load_vos_json(variant(other_size), root, "sot_davis17_val")
    with pytest.raises(ValueError, match="video 5.*do not cover"):
        load_vos_json(variant(short_runs), root, "sot_davis17_val")


def test_the_driver_places_the_mappers_masks(dataset):
    """`InferenceVideoVOS.write_targets_into_annotations_per_clip` on the CPU: the masks of the mapper at [:h, :w] of the right object
    and frame of the padded planes, the boxes normalised by the padded size, the classes, and the frame each object first appears in."""
    from tests import cases
    from univs_amd.inference.video_vos import InferenceVideoVOS
    path, root, _ = dataset
    d = VOSTestMapper(SHORT, MAX, resize="host")(load_vos_json(path, root, "sot_davis17_val")[1])
    h, w = d["instances"][0].image_size
    hp, wp = 32, 32 * -(-w // 32)
    inf = InferenceVideoVOS(**cases.vos_kwargs(dict(Q=8, T=N), clip_stride=1))
    tv = {"task": "sot", "dataset_name": d["dataset_name"], "video_len": N, "inter_image_size": (hp, wp), "instances": d["instances"]}
    inf.write_targets_into_annotations_per_clip([tv], 0, 1)
    assert sorted(tv["ids"]) == [2, 41, 43] and tuple(tv["masks"].shape) == (3, N, hp, wp)
    row = {i: tv["ids"].index(i) for i in tv["ids"]}
    assert [int(tv["first_appear_frame_idxs"][row[i]]) for i in (41, 2, 43)] == [0, 2, 2]     # object 2 is annotated again in frame 2
    assert [int(tv["labels"][row[i]]) for i in (41, 2, 43)] == [2, 1, 2]
    norm = torch.tensor([wp, hp, wp, hp], dtype=torch.float32)
    for f, ann in enumerate(d["instances"]):
        for k, oid in enumerate(ann.ori_ids):
            plane = tv["masks"][row[oid], f]
            assert torch.equal(plane[:h, :w], ann.gt_masks[k].float()) and not plane[h:].any() and not plane[:, w:].any()
            assert torch.equal(tv["mask_logits"][row[oid], f], plane)
            assert torch.equal(tv["boxes"][row[oid], f], ann.gt_boxes.tensor[k] / norm)
    assert not tv["masks"][row[41], 1:].any() and not tv["masks"][row[43], :2].any() and not tv["masks"][:, 3].any()


def test_command_line_arguments_for_vos():
    from univs_amd import run
    base = ["--config-file", "c.yaml", "--weights", "w.pth", "--output-dir", "o"]
    js = ["--json", "j", "--image-root", "r"]
    a = run.parse_args(base + js + ["--dataset-name", "sot_davis17_val", "--davis-root", "D"])
    assert a.vos is True and a.davis_root == "D" and a.pvos_data is None
    a = run.parse_args(base + js + ["--dataset-name", "pvos_viposeg_val", "--pvos-data", "P"])
    assert a.vos is True and a.pvos_data == "P"
    a = run.parse_args(base + js + ["--dataset-name", "sot_ytbvos18_val"])
    assert a.vos is True and run.build_evaluator(a) is None          # only the PNGs are written
    assert run.parse_args(base + js + ["--dataset-name", "ytvis_2021_val"]).vos is False
    assert run.parse_args(base + ["--video-dir", "d"]).vos is False
    for bad in (js + ["--dataset-name", "sot_davis17_val", "--davis-root", "D", "--pvos-data", "P"],     # one evaluator at a time
                js + ["--dataset-name", "sot_davis17_val", "--davis-root", "D", "--gt-json", "g"],
                js + ["--dataset-name", "ytvis_2021_val", "--davis-root", "D"],                          # no VOS data set
                js + ["--dataset-name", "sot_davis17_val", "--gt-json", "g"],
                js + ["--dataset-name", "sot_ytbvos18_val", "--davis-root", "D"],                        # no DAVIS data set
                ["--video-dir", "d", "--pvos-data", "P"]):
        with pytest.raises(SystemExit):
            run.parse_args(base + bad)


def test_clip_offsets_follow_the_schedule_not_the_lengths(tmp_path):
    """`run.write_vos_outputs`: clip c starts at frame c min(clip_stride, num_frames).  With the stride at the clip length a clip that
    is not the last returns one map fewer (the slice of `_finished_frames`), so a running sum of lengths would misplace the rest."""
    from univs_amd import run
    from univs_amd.evaluation.davis import read_results
    assert run.vos_clip_offsets(4, 3, 2) == [0, 2, 4, 6] and run.vos_clip_offsets(3, 3, 5) == [0, 3, 6]
    names = [f"root/JPEGImages/vid/{i:05d}.jpg" for i in range(7)]
    # T = 3, stride 3: clips at 0, 3 and the last one at 6; the first two return T - 1 = 2 maps, frames 2 and 5 are in no clip's output
    outputs = [torch.full((2, 4, 5), 1, dtype=torch.uint8), torch.full((2, 4, 5), 2, dtype=torch.uint8), torch.full((1, 4, 5), 3, dtype=torch.uint8)]
    paths = run.write_vos_outputs(str(tmp_path), [{"file_names": names, "mask_palette": [0] * 768}], outputs, 3, 3)
    assert [os.path.basename(p) for p in paths] == ["00000.png", "00001.png", "00003.png", "00004.png", "00006.png"]
    got = read_results(str(tmp_path / "inference" / "Annotations"), "vid", ["00000", "00001", "00003", "00004", "00006"])
    assert got[:, 0, 0].tolist() == [1, 1, 2, 2, 3]
