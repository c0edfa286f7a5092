"""CPU: `python -m univs_amd.run` on images, end to end with a small synthetic model on the CPU path of the operators
(oracle/cpu_path.py): a folder of jpgs goes in; inference/panoptic/<stem>.png, inference/sem_seg/<stem>.png and
inference/coco_instances_results.json come out, and against a ground truth written from the run's own output PQ and mIoU are 100 -- with
one ground-truth segment relabelled they drop to the values worked out by hand below."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from oracle.cpu_path import cpu_ops
from tests import cases
from tests.frames_cases import frames
from univs_amd import run, synth
from univs_amd.config import load_cfg
from univs_amd.modeling.build import build_model

H, W, N = 48, 72, 3
OFFSET = 20                                                          # (dataset id = contiguous class + 20: the two are never the same number)
CATEGORIES = [{"id": c + OFFSET, "name": "class%d" % c, "isthing": int(c < 80)} for c in range(133)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """(image folder, config file, weights, categories file)."""
    root = tmp_path_factory.mktemp("images")
    os.makedirs(root / "val")
    for i, f in enumerate(frames("noise", N, H, W)):
        Image.fromarray(f).save(root / "val" / f"im{i}.jpg")
    torch.save(cases.clip_table(), root / "clip.pt")
    (root / "cfg.yaml").write_text(f"""MODEL:
  META_ARCHITECTURE: UniVS_Prompt
  MASK_FORMER:
    NUM_OBJECT_QUERIES: 20
    TEST:
      SEMANTIC_ON: True
      INSTANCE_ON: True
      PANOPTIC_ON: True
      OVERLAP_THRESHOLD: 0.8
      OBJECT_MASK_THRESHOLD: 0.05
  UniVS:
    CLIP_CLASS_EMBED_PATH: {root / "clip.pt"}
INPUT:
  SAMPLING_FRAME_NUM: 1
  MIN_SIZE_TEST: 32
  MAX_SIZE_TEST: 64
  LSJ_AUG:
    IMAGE_SIZE: 64
""")
    model = build_model(load_cfg(str(root / "cfg.yaml"))).eval()
    synth.load_synthetic(model)
    torch.save({"model": model.state_dict()}, root / "w.pth")
    (root / "categories.json").write_text(json.dumps({"categories": CATEGORIES}))
    return str(root / "val"), str(root / "cfg.yaml"), str(root / "w.pth"), str(root / "categories.json")


def arguments(tree, out, *more):
    folder, cfg, weights, categories = tree
    return ["--config-file", cfg, "--weights", weights, "--image-dir", folder, "--dataset-name", "coco_panoptic", "--output-dir", str(out),
            "--resize", "host", "--device", "cpu", *more]


@pytest.fixture(scope="module")
def first_run(tree, tmp_path_factory):
    out = tmp_path_factory.mktemp("first")
    with cpu_ops():
        assert run.main(arguments(tree, out, "--categories-json", tree[3])) == 0
    return out


def rgb2id(a):
    a = a.astype(np.int64)
    return a[..., 0] + 256 * a[..., 1] + 65536 * a[..., 2]


def test_image_run_writes_the_three_files(first_run):
    inf = first_run / "inference"
    assert sorted(os.listdir(inf / "panoptic")) == sorted(os.listdir(inf / "sem_seg")) == [f"im{i}.png" for i in range(N)]
    dataset_ids = {c["id"] for c in CATEGORIES}
    for i in range(N):
        pan = np.array(Image.open(inf / "panoptic" / f"im{i}.png"))
        sem = np.array(Image.open(inf / "sem_seg" / f"im{i}.png"))
        assert pan.shape == (H, W, 3) and sem.shape == (H, W) and sem.dtype == np.uint8
        assert set(np.unique(sem).tolist()) <= dataset_ids
    assert len(json.load(open(inf / "predictions.json"))["annotations"]) == N
    records = json.load(open(inf / "coco_instances_results.json"))
    assert len(records) > 0 and {r["image_id"] for r in records} == {f"im{i}" for i in range(N)}
    thing_ids = {c["id"] for c in CATEGORIES if c["isthing"]}
    for r in records:
        assert r["category_id"] in thing_ids and len(r["bbox"]) == 4 and r["segmentation"]["size"] == [H, W] and 0 <= r["score"] <= 1


def ground_truth(first_run, root, relabel=None):
    """COCO-panoptic ground truth from the first run's own panoptic PNGs: the connected labelling as it is (a segment per predicted id,
    its class from the run's predictions.json) and the semantic PNGs as contiguous classes.  `relabel`: (image, k, dataset id)
    gives the k-th listed segment of that image another class."""
    to_contiguous = {c["id"]: i for i, c in enumerate(CATEGORIES)}
    os.makedirs(root / "pan")
    os.makedirs(root / "sem")
    preds = {a["image_id"]: a for a in json.load(open(first_run / "inference" / "predictions.json"))["annotations"]}
    annotations = []
    for i in range(N):
        pan = np.array(Image.open(first_run / "inference" / "panoptic" / f"im{i}.png"))
        Image.fromarray(pan).save(root / "pan" / f"im{i}.png")
        ids = rgb2id(pan)
        segs = [{"id": s["id"], "category_id": s["category_id"], "iscrowd": 0, "area": int((ids == s["id"]).sum())}
                for s in preds[f"im{i}"]["segments_info"]]
        if relabel is not None and relabel[0] == i:
            segs[relabel[1]]["category_id"] = relabel[2]
        annotations.append({"image_id": f"im{i}", "file_name": f"im{i}.png", "segments_info": segs})
        sem = np.array(Image.open(first_run / "inference" / "sem_seg" / f"im{i}.png"))
        Image.fromarray(np.vectorize(to_contiguous.get, otypes=[np.uint8])(sem)).save(root / "sem" / f"im{i}.png")
    (root / "gt.json").write_text(json.dumps({"images": [{"id": f"im{i}", "file_name": f"im{i}.jpg"} for i in range(N)],
                                              "annotations": annotations, "categories": CATEGORIES}))
    return str(root / "gt.json"), str(root / "pan"), str(root / "sem"), annotations


def _run_scored(tree, first_run, root, out, relabel=None, *more):
    gt_json, pan_dir, sem_dir, annotations = ground_truth(first_run, root, relabel)
    import contextlib
    import io
    buf = io.StringIO()
    with cpu_ops(), contextlib.redirect_stdout(buf):
        assert run.main(arguments(tree, out, "--pan-gt-json", gt_json, "--truth-dir", pan_dir, "--sem-gt-dir", sem_dir, *more)) == 0
    return json.loads(buf.getvalue().strip().splitlines()[-1]), annotations


def test_a_ground_truth_from_the_runs_own_output_scores_100(tree, first_run, tmp_path):
    res, annotations = _run_scored(tree, first_run, tmp_path / "gt", tmp_path / "out")
    for i in range(N):                                               # the evaluator's PNG is the writer's
        assert (tmp_path / "out" / "inference" / "panoptic" / f"im{i}.png").read_bytes() == (first_run / "inference" / "panoptic" / f"im{i}.png").read_bytes()
    n_segments = sum(len(a["segments_info"]) for a in annotations)
    assert n_segments >= 2                                           # an empty prediction cannot pass
    pq = res["panoptic_seg"]
    present_things = any(CATEGORIES[s["category_id"] - OFFSET]["isthing"] for a in annotations for s in a["segments_info"])
    present_stuff = any(not CATEGORIES[s["category_id"] - OFFSET]["isthing"] for a in annotations for s in a["segments_info"])
    assert pq["PQ"] == pq["SQ"] == pq["RQ"] == 100.0
    for present, suffix in ((present_things, "_th"), (present_stuff, "_st")):
        if present:
            assert pq["PQ" + suffix] == pq["SQ" + suffix] == pq["RQ" + suffix] == 100.0
    text = (tmp_path / "out" / "inference" / "pq-final.txt").read_text()
    assert text.startswith("PQ:100.0000\nSQ:100.0000\nRQ:100.0000\n")
    per_class = (tmp_path / "out" / "inference" / "pq-per-class.txt").read_text()
    tps = sum(int(line.split()[-3]) for line in per_class.splitlines() if line[:4].strip().isdigit())
    assert tps == n_segments >= 1                                    # true positives, one per segment
    sem = res["sem_seg"]
    assert sem["mIoU"] == sem["fwIoU"] == sem["mACC"] == sem["pACC"] == 100.0
    assert os.path.exists(tmp_path / "out" / "inference" / "predictions.json")
    assert os.path.exists(tmp_path / "out" / "inference" / "sem_seg_evaluation.json")


def test_one_relabelled_segment_lowers_the_numbers_to_the_hand_computed_ones(tree, first_run, tmp_path):
    _, _, _, annotations = ground_truth(first_run, tmp_path / "probe")
    # relabel the first segment of image 0 to a class no image predicts
    used = {s["category_id"] for a in annotations for s in a["segments_info"]}
    old = annotations[0]["segments_info"][0]["category_id"]
    new = next(c["id"] for c in CATEGORIES if c["id"] not in used and c["isthing"] == CATEGORIES[old - OFFSET]["isthing"])
    res, annotations = _run_scored(tree, first_run, tmp_path / "gt", tmp_path / "out", (0, 0, new))
    # by hand: every other segment is a true positive of IoU 1.  Class `old` has its tp of the other segments (t of them) and one false
    # positive (the prediction that lost its ground truth); class `new` has one false negative and nothing else.
    per = {}
    for a in annotations:
        for s in a["segments_info"]:
            per.setdefault(s["category_id"], 0)
            per[s["category_id"]] += 1
    t_old = per.get(old, 0)
    pq_c = {c: 1.0 for c in per if c not in (old, new)}
    pq_c[new] = 0.0                                                  # iou 0 / (0 + 0.5 fn)
    pq_c[old] = t_old / (t_old + 0.5)                                # t_old tp of iou 1 and one fp
    rq_c = dict(pq_c)
    sq_c = {c: 1.0 for c in pq_c}
    sq_c[new] = 0.0
    if t_old == 0:
        sq_c[old] = 0.0
    n = len(pq_c)
    pq = res["panoptic_seg"]
    assert pq["PQ"] == 100 * (sum(pq_c[c] for c in CATEGORIES_ORDER(pq_c)) / n)
    assert pq["RQ"] == 100 * (sum(rq_c[c] for c in CATEGORIES_ORDER(rq_c)) / n)
    assert pq["SQ"] == 100 * (sum(sq_c[c] for c in CATEGORIES_ORDER(sq_c)) / n)
    assert pq["PQ"] < 100.0
    assert res["sem_seg"]["mIoU"] == 100.0                           # the semantic ground truth was not touched


def CATEGORIES_ORDER(d):
    """The keys of d in the categories' order: the order pq_average adds in."""
    return [c["id"] for c in CATEGORIES if c["id"] in d]


@pytest.mark.parametrize("argv", [["--image-dir", "x", "--video-dir", "y"], ["--image-dir", "x", "--json", "j", "--image-root", "r"],
                                  ["--image-dir", "x", "--dataset-name", "ytvis_2021_val", "--categories-json", "c"],
                                  ["--image-dir", "x", "--dataset-name", "coco"],
                                  ["--video-dir", "y", "--batch", "2"], ["--video-dir", "y", "--sem-gt-dir", "s"],
                                  ["--image-dir", "x", "--dataset-name", "coco", "--categories-json", "c", "--pan-gt-json", "p"]])
def test_argument_errors(argv):
    with pytest.raises(SystemExit):
        run.parse_args(["--config-file", "f", "--weights", "w", "--output-dir", "o", *argv])


def test_existing_video_arguments_parse_as_before():
    a = run.parse_args(["--config-file", "f", "--weights", "w", "--output-dir", "o", "--video-dir", "d", "--pan-gt-json", "p", "--truth-dir", "t"])
    assert a.image is False and a.vos is False and a.pan_gt_json == "p"
    a = run.parse_args(["--config-file", "f", "--weights", "w", "--output-dir", "o", "--json", "j", "--image-root", "r", "--dataset-name", "vipseg_val",
                        "--pan-gt-json", "p", "--truth-dir", "t"])
    assert a.image is False
    a = run.parse_args(["--config-file", "f", "--weights", "w", "--output-dir", "o", "--dataset-name", "ade20k", "--image-root", "r",
                        "--pan-gt-json", "p", "--truth-dir", "t", "--sem-gt-dir", "s"])
    assert a.image is True
