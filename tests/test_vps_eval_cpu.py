"""CPU: VPQ / STQ from pair tables (univs_amd/evaluation) against what the reference's own scripts recorded on the g26 scenes
(tools/gen_golden_vps_eval.py).  The tables come from `pair_counts_aten` on CPU tensors; the kernel's side is tests/test_vps_eval_gpu.py."""
import os

import numpy as np
import pytest
import torch

from tests import vps_eval_cases as C
from univs_amd.evaluation import pair_counts as pc
from univs_amd.evaluation import vps


def test_pair_counts_aten_against_a_direct_count():
    g = torch.Generator().manual_seed(26)
    gt_ids, pred_ids = torch.tensor([0, 7, 70000, 1 << 23]), torch.tensor([0, 3, 9])
    gt = gt_ids[torch.randint(0, 4, (2, 5, 7), generator=g)].to(torch.int32)
    pred = torch.cat([pred_ids, torch.tensor([123456])])[torch.randint(0, 4, (2, 5, 7), generator=g)].to(torch.int32)
    gt_rgb = torch.from_numpy(C.ids_to_rgb(gt.numpy()))
    counts, unknown = pc.pair_counts_aten(gt_rgb, pred, gt_ids, pred_ids, with_unknown=True)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (2, 5, 4)
    for t in range(2):
        for gi, a in enumerate(gt_ids.tolist()):
            for pi, b in enumerate(pred_ids.tolist() + [123456]):
                assert int(counts[t, gi, pi]) == int(((gt[t] == a) & (pred[t] == b)).sum())
        assert counts[t, 4].sum() == 0
    assert unknown.tolist() == [[-1, 123456], [-1, 123456]]
    assert torch.equal(pc.pair_counts_aten(gt, pred, gt_ids, pred_ids), counts)          # either encoding
    assert torch.equal(pc.pair_counts(gt_rgb, pred, gt_ids, pred_ids)[0], counts)         # CPU tensors: the ATen formulation


@pytest.mark.parametrize("name", C.SCORED)
def test_scores_from_tables(name):
    fx = C.load(name)
    C.check_score(fx, vps.score_tables(C.tables(fx, "cpu"), fx["gt_json"]))


@pytest.mark.parametrize("name", C.ERRORS)
def test_error_scenes_from_files(name, tmp_path):
    fx = C.load(name)
    submit, truth, gt_file = C.write_tree(fx, str(tmp_path))
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        vps.evaluate_vps_files(submit, truth, gt_file, device="cpu")


@pytest.mark.parametrize("name", C.SCORED)
def test_evaluate_vps_files(name, tmp_path):
    fx = C.load(name)
    submit, truth, gt_file = C.write_tree(fx, str(tmp_path))
    score = vps.evaluate_vps_files(submit, truth, gt_file, device="cpu")
    C.check_score(fx, score)
    C.check_files(fx, submit)


def test_command_line(tmp_path, capsys):
    fx = C.load("short")
    submit, truth, gt_file = C.write_tree(fx, str(tmp_path))
    vps.main(["--submit_dir", submit, "--truth_dir", truth, "--pan_gt_json_file", gt_file, "--device", "cpu"])
    C.check_files(fx, submit)
    assert "vpq_all:" in capsys.readouterr().out


@pytest.mark.parametrize("name", ["clean", "crowd_void"])
def test_evaluator_matches_the_file_path_and_reads_no_predicted_png(name, tmp_path, monkeypatch):
    fx = C.load(name)
    score, out_dir, truth, gt_file, opened = C.run_evaluator(fx, str(tmp_path), "cpu", monkeypatch)
    assert not [p for p in opened if "pan_pred" in p], opened
    assert os.path.exists(os.path.join(out_dir, "pred.json"))
    files = vps.evaluate_vps_files(out_dir, truth, gt_file, device="cpu", output_dir=str(tmp_path / "again"))
    assert score["files"] == files["files"]
    for nframes in vps.NFRAMES:
        assert score["vpq"][nframes] == files["vpq"][nframes]
    assert score["stq"]["STQ"] == files["stq"]["STQ"] and score["stq"]["AQ"] == files["stq"]["AQ"]
    assert np.array_equal(score["stq"]["AQ_per_seq"], files["stq"]["AQ_per_seq"]) and score["stq"]["IoU_per_seq"] == files["stq"]["IoU_per_seq"]
    # (not the fixture's numbers: the writer gives two stuff segments of one category one colour, so its pred.json is another one)


def test_evaluator_without_ground_truth_pngs_reads_the_files(tmp_path, monkeypatch):
    """No ground-truth PNG at `process` time: no tables there, `evaluate` takes the file path (and then needs the PNGs)."""
    import shutil
    from PIL import Image
    fx = C.load("short")
    _, truth, gt_file = C.write_tree(fx, str(tmp_path / "tree"))
    later, out_dir = str(tmp_path / "later"), str(tmp_path / "out")
    ev = vps.VPSEvaluator(C.metadata_categories(fx), gt_file, later, out_dir, device="cpu")
    np.random.seed(0)
    for video in fx["gt_json"]["videos"]:
        inputs, outputs = C.vps_outputs(fx, video["video_id"])
        ev.process([inputs], outputs)
    assert ev._tables == {}
    shutil.copytree(truth, later)
    opened, real = [], Image.open
    monkeypatch.setattr(Image, "open", lambda fp, *a, **k: (opened.append(str(fp)), real(fp, *a, **k))[1])
    score = ev.evaluate()
    monkeypatch.undo()
    frames = sum(len(v["images"]) for v in fx["gt_json"]["videos"])
    assert len([p for p in opened if "pan_pred" in p]) == frames and len(opened) == 2 * frames      # every PNG once
    files = vps.evaluate_vps_files(out_dir, truth, gt_file, device="cpu", output_dir=str(tmp_path / "again"))
    assert score["files"] == files["files"] and score["stq"]["STQ"] == files["stq"]["STQ"]
    # with the PNGs there at `process` time: the same score from the tables counted there
    in_process = C.run_evaluator(fx, str(tmp_path / "with"), "cpu")[0]
    assert in_process["files"] == score["files"] and in_process["stq"]["STQ"] == score["stq"]["STQ"]


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    gt, pred, ids = torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError) as e:
        pc.panoptic_pair_counts(gt, pred, ids, ids)
    assert str(e.value) == "panoptic_pair_counts: Not implemented on the CPU (gt on cpu); the HIP extension is the only implementation"
    with pytest.raises(RuntimeError, match="must be uint8 \\[T, H, W, 3\\] or int32 \\[T, H, W\\]"):
        pc.pair_counts_aten(gt.float(), pred, ids, ids)
    with pytest.raises(RuntimeError, match="do not cover the same"):
        pc.pair_counts_aten(gt, torch.zeros(1, 4, 5, dtype=torch.int32), ids, ids)
