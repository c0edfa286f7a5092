"""CPU: evaluation/image.py against the reference's own `vpq_compute_single_core(nframes=1)` + `pq_average` on the g38 scenes
(tests/golden/g38_image_eval_*.npz, recorded by tools/gen_golden_image_eval.py): every per-class (tp, fp, fn, iou) and the nine
numbers, through `PanopticEvaluator.process` and through the files; the three KeyErrors with their text; and `semseg_scores` /
`SemSegEvaluator` on 3-class matrices worked out by hand."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.image_eval_cases import ERRORS, SCORED, Scene, ids_to_rgb
from univs_amd.evaluation import image as ie


def test_the_scenes_are_the_recorded_ones():
    assert SCORED == ["clean", "crowd", "half", "pred_only", "two_of_a_class", "void"]
    assert ERRORS == ["err_json_not_png", "err_png_not_json", "err_unknown_category"]


@pytest.mark.parametrize("name", SCORED)
def test_panoptic_evaluator_reproduces_the_reference(name, tmp_path):
    s = Scene(name, tmp_path)
    ev = ie.PanopticEvaluator(s.gt_json, s.truth_dir, str(tmp_path / "out"), device="cpu")
    ev.reset()
    for item, output in s.driver_io():
        ev.process([item], [output])
    out = ev.evaluate()
    assert list(out) == ["panoptic_seg"] and list(out["panoptic_seg"]) == ["PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st"]
    s.check(out["panoptic_seg"], ev.last)
    # what it wrote: the PNG holds the ids, the record the dataset ids; scoring those files gives the same numbers
    inf = tmp_path / "out" / "inference"
    for i in s.image_ids:
        assert np.array_equal(np.array(Image.open(inf / "panoptic" / f"{i}.png")), ids_to_rgb(s.z["pred_" + i]))
    written = json.load(open(inf / "predictions.json"))["annotations"]
    for w, p in zip(written, s.pred["annotations"]):
        assert w["image_id"] == p["image_id"] and w["file_name"] == p["file_name"]
        assert [(x["id"], x["category_id"]) for x in w["segments_info"]] == [(x["id"], x["category_id"]) for x in p["segments_info"]]
        assert all(isinstance(x["isthing"], bool) for x in w["segments_info"])
    again = ie.evaluate_panoptic_files(str(inf / "panoptic"), s.gt_json, s.truth_dir, device="cpu")
    assert json.dumps(again["panoptic_seg"]) == json.dumps(out["panoptic_seg"])
    assert (inf / "pq-final.txt").read_text() == ie.pq_final_text(out["panoptic_seg"])


def test_the_scenes_show_what_they_are_named_for(tmp_path):
    def per_class(name):
        s = Scene(name, tmp_path / name, files=True)
        ev = ie.PanopticEvaluator(s.gt_json, s.truth_dir, str(tmp_path / name), device="cpu")
        for rec in s.pred["annotations"]:
            p = torch.as_tensor(np.array(Image.open(os.path.join(s.panoptic_dir, rec["file_name"]))))
            ev._tables[rec["image_id"]] = ev.count(rec["image_id"], rec, p)
        return ie.score_panoptic(ev._gt, ev._tables, ev.categories)[1]["per_class"]
    half = per_class("half")[7]
    assert (half["tp"], half["fp"], half["fn"]) == (0, 1, 1)         # IoU exactly 0.5 is no match
    void = per_class("void")[9]
    assert (void["tp"], void["fp"], void["fn"]) == (0, 0, 0)         # more than half on VOID: not a false positive
    crowd = per_class("crowd")[7]
    assert (crowd["tp"], crowd["fp"], crowd["fn"]) == (1, 1, 0)      # on the crowd: ignored; half off it: a false positive; the crowd: no fn
    only = per_class("pred_only")[9]
    assert (only["tp"], only["fp"], only["fn"]) == (0, 1, 0)
    two = per_class("two_of_a_class")[7]
    assert (two["tp"], two["fp"], two["fn"]) == (1, 1, 1)


@pytest.mark.parametrize("name", ERRORS)
def test_the_three_key_errors_keep_their_text(name, tmp_path):
    s = Scene(name, tmp_path, files=True)
    assert str(s.z["error"]) == "KeyError"
    with pytest.raises(KeyError) as e:
        ie.evaluate_panoptic_files(s.panoptic_dir, s.gt_json, s.truth_dir, device="cpu")
    assert e.value.args[0] == str(s.z["error_text"])


def test_a_prediction_of_another_size_is_the_reference_s_assertion(tmp_path):
    s = Scene("half", tmp_path)
    ev = ie.PanopticEvaluator(s.gt_json, s.truth_dir, str(tmp_path / "out"), device="cpu")
    item, output = s.driver_io()[0]
    output["panoptic_seg"] = (output["panoptic_seg"][0][:-1], output["panoptic_seg"][1])
    with pytest.raises(AssertionError, match="Dismatch shape"):
        ev.process([item], [output])
    with pytest.raises(KeyError, match="no annotation"):
        ev.count("nope", s.pred["annotations"][0], s.z["pred_a"])


# ---- mIoU: matrices worked out by hand ------------------------------------------------------------------------------------------------
def test_semseg_scores_on_a_hand_worked_matrix():
    # rows = ground truth (row 3: ignored pixels), columns = prediction
    conf = np.array([[6, 2, 0, 0],
                     [1, 3, 0, 0],
                     [0, 4, 0, 0],
                     [5, 5, 5, 0]])
    r = ie.semseg_scores(conf, ["a", "b", "c"])
    # tp = (6, 3, 0); pos_gt = (8, 4, 4); pos_pred = (7, 9, 0); union = (9, 10, 4)
    assert r["IoU-a"] == 100 * (6 / 9) and r["IoU-b"] == 100 * (3 / 10) and r["IoU-c"] == 0.0
    assert r["ACC-a"] == 100 * (6 / 8) and r["ACC-b"] == 100 * (3 / 4) and r["ACC-c"] == 0.0
    assert r["mIoU"] == 100 * ((6 / 9 + 3 / 10 + 0.0) / 3)
    assert r["mACC"] == 100 * ((6 / 8 + 3 / 4 + 0.0) / 3)
    assert r["fwIoU"] == 100 * (6 / 9 * (8 / 16) + 3 / 10 * (4 / 16) + 0.0 * (4 / 16))
    assert r["pACC"] == 100 * (9 / 16)
    assert list(r) == ["mIoU", "fwIoU", "IoU-a", "IoU-b", "IoU-c", "mACC", "pACC", "ACC-a", "ACC-b", "ACC-c"]


def test_semseg_scores_leave_out_a_class_without_ground_truth_and_one_with_union_zero():
    # class b has no ground-truth pixel (pos_gt == 0) though it is predicted; class c occurs on neither side (union 0)
    conf = np.array([[5, 3, 0, 0],
                     [0, 0, 0, 0],
                     [0, 0, 0, 0],
                     [0, 2, 0, 0]])
    r = ie.semseg_scores(conf, ["a", "b", "c"])
    assert r["IoU-a"] == 100 * (5 / 8) and np.isnan(r["IoU-b"]) and np.isnan(r["IoU-c"])
    assert r["ACC-a"] == 100 * (5 / 8) and np.isnan(r["ACC-b"]) and np.isnan(r["ACC-c"])
    assert r["mIoU"] == 100 * (5 / 8) and r["mACC"] == 100 * (5 / 8) and r["fwIoU"] == 100 * (5 / 8) and r["pACC"] == 100 * (5 / 8)


def test_semseg_evaluator_counts_images_of_two_sizes_from_labels_and_from_scores(tmp_path):
    K = 3
    rng = np.random.default_rng(0)
    ev = ie.SemSegEvaluator(str(tmp_path), K, 255, ["a", "b", "c"], str(tmp_path / "out"), device="cpu")
    total = np.zeros((K + 1, K + 1), np.int64)
    for n, (h, w) in enumerate(((7, 9), (12, 5))):
        gt = rng.integers(0, K, (h, w)).astype(np.uint8)
        gt[0, :3] = 255
        pred = rng.integers(0, K, (h, w)).astype(np.uint8)
        Image.fromarray(gt).save(tmp_path / f"im{n}.png")
        g = np.where(gt == 255, K, gt).astype(np.int64)
        np.add.at(total, (g.ravel(), pred.ravel().astype(np.int64)), 1)
        item = {"file_names": [f"/x/im{n}.jpg"], "image_id": f"im{n}"}
        if n == 0:
            ev.process([item], [{"sem_seg_labels": torch.as_tensor(pred)}])
        else:                                                        # an output that only holds scores: argmax first
            scores = torch.zeros((K, h, w))
            scores.scatter_(0, torch.as_tensor(pred).long()[None], 1.0)
            ev.process([item], [{"sem_seg": scores}])
    out = ev.evaluate()
    assert list(out) == ["sem_seg"] and json.dumps(out["sem_seg"]) == json.dumps(ie.semseg_scores(total, ["a", "b", "c"]))
    assert json.load(open(tmp_path / "out" / "inference" / "sem_seg_evaluation.json")) == json.loads(json.dumps(out["sem_seg"]))
    # a stray ground-truth value is the ValueError, raised at evaluate()
    Image.fromarray(np.full((4, 4), 9, np.uint8)).save(tmp_path / "bad.png")
    ev.process([{"file_names": ["/x/bad.jpg"]}], [{"sem_seg_labels": torch.zeros((4, 4), dtype=torch.uint8)}])
    with pytest.raises(ValueError, match="16 ground-truth pixels"):
        ev.evaluate()


def test_command_line_scores_files_on_disk(tmp_path, capsys):
    s = Scene("clean", tmp_path, files=True)
    r = ie.main(["--panoptic_dir", s.panoptic_dir, "--pan_gt_json", s.gt_json, "--truth_dir", s.truth_dir, "--device", "cpu"])
    s.check(r["panoptic_seg"], _res_of(s, tmp_path))
    assert capsys.readouterr().out.startswith("PQ:")
    os.makedirs(tmp_path / "sem")
    os.makedirs(tmp_path / "semgt")
    a = np.array([[0, 1], [2, 255]], np.uint8)
    Image.fromarray(a).save(tmp_path / "semgt" / "x.png")
    Image.fromarray(np.array([[0, 1], [1, 0]], np.uint8)).save(tmp_path / "sem" / "x.png")
    r = ie.main(["--sem_dir", str(tmp_path / "sem"), "--sem_gt_dir", str(tmp_path / "semgt"), "--num_classes", "3", "--device", "cpu"])
    assert r["sem_seg"]["pACC"] == 100 * (2 / 3) and r["sem_seg"]["mIoU"] == 100 * ((1 + 1 / 2 + 0) / 3)
    with pytest.raises(SystemExit):
        ie.main(["--panoptic_dir", "x", "--sem_dir", "y"])


def _res_of(s, tmp_path):
    ev = ie.PanopticEvaluator(s.gt_json, s.truth_dir, str(tmp_path / "again"), device="cpu")
    for item, output in s.driver_io():
        ev.process([item], [output])
    ev.evaluate()
    return ev.last
