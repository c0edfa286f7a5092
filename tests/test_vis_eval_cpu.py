"""CPU: the YouTube-VIS scorer (univs_amd/evaluation/ytvis.py over vis_counts.py) against what the reference's YTVOS / YTVOSeval /
YTVISEvaluator recorded for the g29 scenes (tools/gen_golden_vis_eval.py) -- exact equality of float64 tables --, the run decoder
against the per-character coder of results.py, and the ATen overlap against a dense AND-count.  Nothing here reads the reference."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vis_eval_cases as C
from univs_amd import evaluation
from univs_amd.evaluation import vis_counts as vc
from univs_amd.evaluation import ytvis
from univs_amd.inference import results as R

CPU = torch.device("cpu")


def _fixtures():
    return {name: C.load(name) for name in C.SCORED}


@pytest.fixture(scope="module")
def scenes():
    return _fixtures()


@pytest.mark.parametrize("name", C.SCORED)
def test_scene_equals_the_reference(scenes, name):
    C.check_scene(scenes[name], CPU)


@pytest.mark.parametrize("name", C.ERRORS)
def test_error_scene_raises_the_recorded_type(name):
    fx = C.load(name)
    ev = ytvis.YTVISEvaluator(fx["gt"], device=CPU)
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        ytvis.evaluate_predictions_on_ytvis(ev._dataset, fx["results"], device=CPU)


def _check_runs(rles, H, W):
    """runs_from_rles against rle_counts / rle_decode, mask by mask."""
    runs = vc.runs_from_rles(rles, H, W)
    assert all(x.dtype == torch.int32 for x in runs) and runs.starts.numel() == len(rles) + 1
    areas = runs.areas()
    for i, r in enumerate(rles):
        s, e = int(runs.starts[i]), int(runs.starts[i + 1])
        if not r:
            assert s == e and int(areas[i]) == 0
            continue
        counts = np.asarray(r["counts"], np.int64) if isinstance(r["counts"], list) else R.rle_counts(r)
        assert np.array_equal(runs.bounds[s:e].numpy(), np.cumsum(counts))
        fg = np.where(np.arange(len(counts)) % 2 == 1, counts, 0)
        assert np.array_equal(runs.ones[s:e].numpy(), np.cumsum(fg))
        if not isinstance(r["counts"], list):
            assert int(areas[i]) == int(R.rle_decode(r).sum()) == R.rle_area(r)
    return runs


def test_runs_agree_with_the_string_coder_on_every_mask_of_every_scene(scenes):
    n = 0
    for fx in scenes.values():
        size = {v["id"]: (v["height"], v["width"]) for v in fx["gt"]["videos"]}
        for rec in fx["gt"]["annotations"] + fx["results"]:
            _check_runs(rec["segmentations"], *size[rec["video_id"]])
            n += len(rec["segmentations"])
    assert n > 400


def test_runs_of_hand_made_codes():
    H, W = 5, 7
    hw = H * W
    lead = np.zeros((H, W), bool)
    lead[0, 0] = lead[2, 3] = True                                      # a leading zero-length run
    last = np.zeros((H, W), bool)
    last[-1, -1] = True                                                 # a single last pixel
    masks = torch.from_numpy(np.stack([lead, np.ones((H, W), bool), np.zeros((H, W), bool), last]))
    rles = R.rle_encode_masks(masks)
    assert R.rle_counts(rles[0])[0] == 0 and R.rle_counts(rles[1]).tolist() == [0, hw] and R.rle_counts(rles[2]).tolist() == [hw]
    assert R.rle_counts(rles[3]).tolist() == [hw - 1, 1]
    runs = _check_runs(rles + [None, {"size": [H, W], "counts": [0, hw]}, {"size": [H, W], "counts": [hw]}], H, W)
    assert runs.areas().tolist() == [2, hw, 0, 1, 0, hw, 0]
    # counts after the third are stored as differences to the count two places back: 30, 2, 40, 1, 5, 3, ... needs negative ones
    H, W = 40, 50
    counts = [30, 2, 40, 1, 5, 3, 900, 700, 2, 1]
    counts.append(H * W - sum(counts))
    flat = np.repeat(np.arange(len(counts)) % 2, counts).astype(bool)
    rle = R.rle_encode_masks(torch.from_numpy(flat.reshape(W, H).T.copy()[None]))[0]
    assert R.rle_counts(rle).tolist() == counts
    runs = _check_runs([rle, {"size": [H, W], "counts": rle["counts"].encode("ascii")}], H, W)
    assert runs.bounds[:len(counts)].tolist() == np.cumsum(counts).tolist()


def test_bad_codes_raise():
    H, W = 6, 8
    good = R.rle_encode_masks(torch.ones(1, H, W, dtype=torch.bool))[0]
    with pytest.raises(ValueError, match="video 17"):
        vc.runs_from_rles([good, {"size": [H, W], "counts": [3, 4]}], H, W, video=17)             # 7 of 48 pixels
    with pytest.raises(ValueError, match="video 17"):
        vc.runs_from_rles([R.rle_encode_masks(torch.ones(1, H, W + 1, dtype=torch.bool))[0]], H, W, video=17)
    with pytest.raises(ValueError, match="video 17"):
        vc.runs_from_rles([{"size": [H, W], "counts": good["counts"][:-1] + "00"}], H, W, video=17)
    with pytest.raises(NotImplementedError, match="polygon"):
        vc.runs_from_rles([[[1.0, 1.0, 4.0, 1.0, 4.0, 4.0]]], H, W)
    # through the scorer: the size of a result mask is not its video's
    fx = C.load("crowd")
    fx["results"][0]["segmentations"][1] = good
    with pytest.raises(ValueError, match="video 1"):
        ytvis.evaluate_predictions_on_ytvis(fx["gt"], fx["results"], device=CPU)
    fx = C.load("crowd")
    fx["gt"]["annotations"][0]["segmentations"][0] = [[1.0, 1.0, 4.0, 1.0, 4.0, 4.0]]
    with pytest.raises(NotImplementedError):
        ytvis.evaluate_predictions_on_ytvis(fx["gt"], fx["results"], device=CPU)


@pytest.mark.parametrize("D,G,T,H,W", [(5, 3, 3, 37, 53), (1, 1, 1, 4, 3), (2, 4, 2, 16, 9)])
def test_aten_overlap_equals_the_dense_count(D, G, T, H, W):
    d, g = C.blobs(D, T, H, W, 1), C.blobs(G, T, H, W, 2)
    d[0, 0] = True                                                      # a full mask, an empty one, absent ones
    g[-1, -1] = False
    d_absent, g_absent = ((D * T - 1,) if D * T > 1 else ()), ((0,) if G * T > 1 else ())
    got = vc.vis_overlap_aten(C.runs_of(d, d_absent), C.runs_of(g, g_absent), T, H, W)
    assert got.dtype == torch.int32 and got.shape == (D, G, T)
    assert torch.equal(got.to(torch.int64), C.brute(d, g, d_absent, g_absent))
    assert torch.equal(vc.vis_overlap(C.runs_of(d, d_absent), C.runs_of(g, g_absent), T, H, W), got)       # CPU tensors: the ATen path
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        vc.vis_video_overlap(C.runs_of(d), C.runs_of(g), T, H, W)


def test_shared_segmentation_lists_are_counted_once_and_the_dict_form_is_encoded():
    fx = C.load("clean")
    H, W = fx["gt"]["videos"][0]["height"], fx["gt"]["videos"][0]["width"]
    first = [r for r in fx["results"] if r["video_id"] == 1]
    twin = dict(first[0], score=0.123, category_id=2)                   # shares first[0]'s list, as the records of one entity do
    e = ytvis.YTVISEval(fx["gt"], first + [twin], device=CPU)
    assert int(e.dt_runs[1][0].starts.numel()) - 1 == len(first) * len(first[0]["segmentations"])
    assert e.dt_runs[1][1].tolist() == list(range(len(first))) + [0]
    # pred_scores / pred_labels / pred_masks: the masks are encoded as rle_encode_masks does
    masks = [torch.from_numpy(np.stack([R.rle_decode(s) for s in r["segmentations"]])).bool() for r in first]
    ev = ytvis.YTVISEvaluator(fx["gt"], device=CPU)
    ev.process([{"video_id": 1, "height": H, "width": W}], {"pred_scores": [r["score"] for r in first],
                                                             "pred_labels": [r["category_id"] for r in first], "pred_masks": masks})
    assert [{k: r[k] for k in ("video_id", "score", "category_id", "segmentations")} for r in ev._predictions] == \
           [{k: r[k] for k in ("video_id", "score", "category_id", "segmentations")} for r in first]
    with pytest.raises(ValueError):
        ev.process(None, 3)


def test_category_unmapping_and_output_files(tmp_path):
    fx = C.load("absent_category")
    mapped = [dict(r, category_id=r["category_id"] - 1) for r in fx["results"]]
    ev = ytvis.YTVISEvaluator(fx["gt"], thing_classes=fx["class_names"], output_dir=str(tmp_path), device=CPU,
                              thing_dataset_id_to_contiguous_id={1: 0, 2: 1, 3: 2})
    ev.process(None, mapped)
    res = ev.evaluate()
    assert C.same(list(res["segm"].values()), fx["derived_values"])
    assert [r["category_id"] for r in json.load(open(tmp_path / "results.json"))] == [r["category_id"] for r in fx["results"]]
    assert len(torch.load(tmp_path / "instances_predictions.pth", weights_only=False)) == len(mapped)
    ev.reset()
    assert ev.evaluate() == {}


def test_cli_prints_the_twelve_lines(tmp_path):
    fx = C.load("area_ranges")
    (tmp_path / "gt.json").write_text(str(fx["gt_json"]))
    (tmp_path / "results.json").write_text(str(fx["results_json"]))
    out = subprocess.run([sys.executable, "-m", "univs_amd.evaluation.ytvis", "--gt_json", str(tmp_path / "gt.json"), "--results",
                          str(tmp_path / "results.json"), "--device", "cpu"], check=True, capture_output=True, text=True).stdout
    assert out.splitlines() == [str(s) for s in fx["lines"]]


def test_names_are_exported():
    for n in ("YTVISEvaluator", "YTVISEval", "runs_from_rles", "vis_overlap", "vis_overlap_aten", "vis_video_overlap"):
        assert n in evaluation.__all__ and callable(getattr(evaluation, n))
