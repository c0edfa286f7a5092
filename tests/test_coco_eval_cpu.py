"""CPU: COCO mask AP (univs_amd/evaluation/coco.py).  The matcher is YTVISEval's, which is pinned to the reference's ytvoseval.py: a
crowd-free scene scored as a one-frame YouTube-VIS file gives the same area-independent numbers bit for bit.  Polygons and RLE give
identical results; the area bounds are inclusive; a crowd region worked by hand; the size refusal; the evaluator's file; the
--inst-gt-json argument of run.py."""
import argparse
import json

import numpy as np
import pytest

from tests import coco_scene
from univs_amd import run
from univs_amd.evaluation import coco
from univs_amd.evaluation.ytvis import evaluate_predictions_on_ytvis


@pytest.fixture(scope="module")
def scored():
    dataset, results = coco_scene.scene()
    return coco.evaluate_predictions_on_coco(dataset, results, "cpu")


def test_the_matcher_is_the_one_pinned_to_the_reference(scored):
    dataset, results = coco_scene.scene()
    vis = evaluate_predictions_on_ytvis(*coco_scene.as_ytvis(dataset, results), device="cpu")
    assert len(dataset["annotations"]) >= 10 and len(results) >= 15
    assert np.array_equal(scored.stats[[0, 1, 2, 6, 7, 8]], vis.stats[[0, 1, 2, 6, 7, 8]])       # AP, AP50, AP75, AR1, AR10, AR100
    assert 0 < scored.stats[0] < scored.stats[1] <= 1
    assert np.array_equal(scored.eval["precision"][..., 0, :], vis.eval["precision"][..., 0, :])
    assert np.array_equal(scored.eval["recall"][..., 0, :], vis.eval["recall"][..., 0, :])
    assert scored.summary[:3] == vis.summary[:3] and len(scored.summary) == 12


def test_polygons_and_rle_give_identical_results(scored):
    dataset, results = coco_scene.scene()
    rle = coco.evaluate_predictions_on_coco(coco_scene.with_rle_ground_truth(dataset), results, "cpu")
    assert all(np.array_equal(a, b) for a, b in zip(scored.gt_runs, rle.gt_runs))
    assert np.array_equal(scored.stats, rle.stats) and np.array_equal(scored.eval["precision"], rle.eval["precision"])


def _one(area, segm_gt, segm_dt, size=(80, 80), iscrowd=0):
    ds = {"images": [{"id": 1, "height": size[0], "width": size[1]}], "categories": [{"id": 1, "name": "a"}],
          "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "segmentation": segm_gt, "area": area, "iscrowd": iscrowd}]}
    return ds, [{"image_id": 1, "category_id": 1, "segmentation": s, "score": 0.9 - 0.1 * i} for i, s in enumerate(segm_dt)]


def _rect(x0, y0, x1, y1):
    return [float(v) for v in (x0, y0, x1, y0, x1, y1, x0, y1)]


def _full(ap):
    """An AP of one: COCOeval's precision is tp / (fp + tp + eps), so its mean stays a rounding below 1."""
    return 1 - 1e-12 < ap <= 1


def test_area_bounds_are_inclusive():
    sq = [_rect(8, 8, 40, 40)]                                                            # 32 x 32 = 1024 pixels
    e = coco.evaluate_predictions_on_coco(*_one(1024, sq, [{"size": [80, 80], "counts": coco_scene.counts_of(sq, 80, 80)}]), "cpu")
    assert e._dt_area.tolist() == [1024] and _full(e.stats[3]) and _full(e.stats[4]) and e.stats[5] == -1     # small and medium, not large
    e = coco.evaluate_predictions_on_coco(*_one(1025, sq, [{"size": [80, 80], "counts": coco_scene.counts_of(sq, 80, 80)}]), "cpu")
    assert e.stats[3] == -1 and _full(e.stats[4])                                          # the json's area decides for a ground truth
    big = [_rect(0, 0, 96, 96)]
    e = coco.evaluate_predictions_on_coco(*_one(9216, big, [big], size=(100, 100)), "cpu")
    assert _full(e.stats[4]) and _full(e.stats[5]) and e.stats[3] == -1
    assert e.stats[9:].tolist() == [-1, 1.0, 1.0]                                         # (the recalls are exact)


def test_two_detections_inside_a_crowd_region_are_matched_and_ignored():
    h = w = 60
    crowd = {"size": [h, w], "counts": coco_scene.counts_of([_rect(5, 5, 45, 45)], h, w)}
    ds, res = _one(1600, crowd, [[_rect(10, 10, 20, 20)], [_rect(25, 25, 40, 44)], [_rect(50, 50, 58, 58)]], size=(h, w), iscrowd=1)
    ds["annotations"].append({"id": 2, "image_id": 1, "category_id": 1, "segmentation": [_rect(50, 50, 58, 58)], "area": 64, "iscrowd": 0})
    e = coco.evaluate_predictions_on_coco(ds, res, "cpu")
    assert e.ious[1, 1].tolist() == [[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]]                  # I / A_d against the crowd, rows by score
    ev = e.eval_vids[0]                                                                   # category 1, all areas, image 1
    assert ev["gtIds"] == [2, 1] and ev["gtIgnore"].tolist() == [0, 1]                    # the crowd region last
    assert (ev["dtMatches"] == np.array([[1, 1, 2]] * 10)).all()                          # both matched to the crowd, at every threshold
    assert (ev["dtIgnore"] == np.array([[True, True, False]] * 10)).all()
    assert _full(e.stats[0]) and e.stats[8] == 1.0                                        # the ignored ones cost nothing
    # one detection half outside the crowd: I / A_d = 0.5 exactly, matched from the first threshold only
    ds, res = _one(1600, crowd, [[_rect(35, 10, 55, 20)]], size=(h, w), iscrowd=1)
    e = coco.evaluate_predictions_on_coco(ds, res, "cpu")
    assert e.ious[1, 1].tolist() == [[0.5]] and e.eval_vids[0]["dtMatches"][:, 0].tolist() == [1.0] + [0.0] * 9


def test_a_mask_of_another_size_names_its_image():
    sq = [_rect(8, 8, 40, 40)]
    ds, res = _one(1024, sq, [{"size": [80, 81], "counts": [0, 6480]}])
    with pytest.raises(ValueError, match="image 1, result 1: a mask of size \\[80, 81\\] on an image of \\[80, 80\\]"):
        coco.COCOSegmEval(ds, res, "cpu")
    ds, res = _one(1024, {"size": [81, 80], "counts": [0, 6480]}, [sq])
    with pytest.raises(ValueError, match="image 1, annotation 1: a mask of size"):
        coco.COCOSegmEval(ds, res, "cpu")
    ds, res = _one(1024, [[1, 2, 3, 4, 5]], [sq])
    with pytest.raises(ValueError, match="image 1, annotation 1, polygon 0: .*odd count"):
        coco.COCOSegmEval(ds, res, "cpu")


def test_the_evaluator_writes_its_file_and_the_command_line_prints_it(tmp_path, capsys, scored):
    dataset, results = coco_scene.scene()
    by_name = [dict(r, image_id=f"{r['image_id']:06d}") for r in results]                  # an --image-dir run names images by their files
    ev = coco.COCOInstanceEvaluator(dataset, str(tmp_path / "out"), "cpu")
    ev.process(by_name[:7])
    ev.process(by_name[7:])
    out = ev.evaluate()
    assert list(out) == ["segm"] and list(out["segm"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP-cat", "AP-dog", "AP-cup"]
    assert out["segm"]["AP"] == scored.stats[0] * 100
    lines = (tmp_path / "out" / "coco-segm-ap.txt").read_text().splitlines()
    assert lines == scored.summary and len(lines) == 12
    ev.reset()
    assert ev._predictions == []
    with pytest.raises(ValueError, match="neither an image id nor a file name"):
        ev.process([dict(results[0], image_id="nowhere")])
        ev.evaluate()
    g, r = tmp_path / "gt.json", tmp_path / "results.json"
    g.write_text(json.dumps(dataset))
    r.write_text(json.dumps(results))
    capsys.readouterr()
    assert coco.main(["--gt_json", str(g), "--results", str(r), "--device", "cpu"]) == 0
    assert capsys.readouterr().out.splitlines() == scored.summary


def test_run_inst_gt_json_arguments(tmp_path, capsys, scored):
    dataset, results = coco_scene.scene()
    g = tmp_path / "instances.json"
    g.write_text(json.dumps(dataset))
    base = ["--config-file", "F", "--weights", "W", "--output-dir", str(tmp_path)]
    image = base + ["--image-dir", str(tmp_path), "--dataset-name", "coco", "--categories-json", str(g)]
    assert run.parse_args(image + ["--inst-gt-json", str(g)]).inst_gt_json == str(g)
    assert not hasattr(run.parse_args(image), "inst_gt_json")                             # (the other runs' namespaces stay what they were)
    for argv in (image + ["--inst-gt-json", str(tmp_path / "missing.json")],                                   # no such file
                 base + ["--video-dir", str(tmp_path), "--inst-gt-json", str(g)],                              # a video run
                 base + ["--image-dir", str(tmp_path), "--class-names", str(g), "--inst-gt-json", str(g)]):    # a vocabulary of names
        with pytest.raises(SystemExit):
            run.parse_args(argv)
    capsys.readouterr()
    args = argparse.Namespace(inst_gt_json=str(g), output_dir=str(tmp_path), device="cpu")
    out = run.score_instances(args, results, {"panoptic_seg": {"PQ": 1.0}})
    assert out["panoptic_seg"] == {"PQ": 1.0} and out["segm"]["AP"] == scored.stats[0] * 100
    assert capsys.readouterr().out.splitlines() == scored.summary
    assert (tmp_path / "inference" / "coco-segm-ap.txt").read_text().splitlines() == scored.summary
    assert run.score_instances(args, [], {"x": 1}) == {"x": 1}
