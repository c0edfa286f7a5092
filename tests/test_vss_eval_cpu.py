"""CPU: the VSS scoring (univs_amd/evaluation/vss.py over vss_counts.py's ATen formulation) against what the reference's own scripts
recorded on the g27 scenes (tools/gen_golden_vss_eval.py): counts equal, texts byte-identical."""
import os

import numpy as np
import pytest
import torch

from tests import vss_eval_cases as C
from univs_amd.evaluation import vss
from univs_amd.evaluation import vss_counts as vc


@pytest.mark.parametrize("name", C.SCORED)
def test_scores_from_counts(name):
    fx = C.load(name)
    C.check_score(fx, vss.score_counts(C.video_counts(fx, "cpu"), fx["split_file"]))


@pytest.mark.parametrize("name", C.SCORED)
def test_evaluate_vss_files(name, tmp_path):
    fx = C.load(name)
    submit, data = C.write_tree(fx, str(tmp_path))
    C.check_score(fx, vss.evaluate_vss_files(submit, data, fx["split_file"], device="cpu"))
    C.check_files(fx, submit)                            # the scripts' place: the submit directory


def test_evaluate_vss_files_output_dir_and_command_line(tmp_path, capsys):
    fx = C.load("clean")
    submit, data = C.write_tree(fx, str(tmp_path))
    out = str(tmp_path / "scores")
    vss.evaluate_vss_files(submit, data, fx["split_file"], device="cpu", output_dir=out)
    C.check_files(fx, out)
    assert not os.path.exists(os.path.join(submit, "miou-final.txt"))
    r = vss.main(["--submit_dir", submit, "--data_dir", data, "--split_file", fx["split_file"], "--device", "cpu"])
    C.check_score(fx, r)
    C.check_files(fx, submit)
    assert fx["file_texts"].tolist()[0] in capsys.readouterr().out


@pytest.mark.parametrize("name", C.ERRORS)
def test_evaluator_raises_the_error_scenes_from_evaluate(name, tmp_path):
    """`process` takes every video (an overflowing count, another size, a missing frame: each sends the video to the files); the
    recorded error comes from `evaluate`, as the reference's."""
    fx = C.load(name)
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        C.run_evaluator(fx, str(tmp_path), "cpu")
    assert not os.path.exists(str(tmp_path / "tree" / "run" / "miou-final.txt"))


def test_evaluator_keeps_no_counts_of_a_video_it_cannot_score_in_process(tmp_path):
    for name, video in (("err_overflow", "v_o"), ("err_size_mismatch", "v_s"), ("err_missing_pred", "v_m")):
        fx = C.load(name)
        submit, data = C.write_tree(fx, str(tmp_path / name), predictions=False)
        ev = vss.VSSEvaluator(C.CONTIGUOUS_TO_DATASET, 255, C.NUM_CLASSES, data, fx["split_file"], submit, device="cpu")
        inputs, outputs = C.vss_outputs(fx, video)
        ev.process([inputs], outputs)
        assert ev._counts == {}, name


def test_an_empty_split_scores_the_zero_matrix(tmp_path):
    data, submit = tmp_path / "VSPW", tmp_path / "submit"
    data.mkdir()
    submit.mkdir()
    (data / "val.txt").write_text("")
    r = vss.evaluate_vss_files(str(submit), str(data), "val.txt", device="cpu")
    assert r["confusion"].shape == (124, 124) and not r["confusion"].any()
    assert r["files"] == {"miou-final.txt": "Acc:nan, Acc_class:nan, mIoU:nan, fwIoU: 0.0",
                          "vc8-final.txt": "VC8 score: nan on val.txt set", "vc16-final.txt": "VC16 score: nan on val.txt set"}


@pytest.mark.parametrize("name", C.EVALUATOR_SCORED)
def test_evaluator_scores_in_process_and_writes_beside_its_directory(name, tmp_path, monkeypatch):
    fx = C.load(name)
    score, submit, data, opened = C.run_evaluator(fx, str(tmp_path), "cpu", monkeypatch)
    C.check_score(fx, score)
    parent = os.path.dirname(submit)
    C.check_files(fx, parent)                            # the evaluator's place: the parent of its output directory
    assert not os.path.exists(os.path.join(submit, "miou-final.txt"))
    assert opened == [], "evaluate() re-read files of videos that process() had counted"
    again = vss.evaluate_vss_files(submit, data, fx["split_file"], device="cpu", output_dir=str(tmp_path / "again"))
    assert again["files"] == score["files"] and np.array_equal(again["confusion"], score["confusion"])


def test_evaluator_scores_an_unprocessed_video_from_the_files(tmp_path, monkeypatch):
    fx = C.load("clean")
    submit, data = C.write_tree(fx, str(tmp_path))       # every prediction is on the disk already
    ev = vss.VSSEvaluator(C.CONTIGUOUS_TO_DATASET, 255, C.NUM_CLASSES, data, fx["split_file"], submit, device="cpu")
    ev.reset()
    ev.process([C.vss_outputs(fx, "v_b")[0]], C.vss_outputs(fx, "v_b")[1])
    assert sorted(ev._counts) == ["v_b"]
    C.check_score(fx, ev.evaluate())


def test_evaluator_refuses_the_rescaled_miou():
    with pytest.raises(NotImplementedError):
        vss.VSSEvaluator(C.CONTIGUOUS_TO_DATASET, 255, C.NUM_CLASSES, "data", "val.txt", "out", eval_miou_res=480)


@pytest.mark.parametrize("name", C.ERRORS)
def test_error_scenes(name, tmp_path):
    fx = C.load(name)
    submit, data = C.write_tree(fx, str(tmp_path))
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        vss.evaluate_vss_files(submit, data, fx["split_file"], device="cpu")


def test_overflow_flag_names_the_largest_cell():
    fx = C.load("err_overflow")
    g, p = torch.from_numpy(fx["gt_v_o"]), torch.from_numpy(fx["pred_v_o"])
    confusion, _, overflow = vc.vss_counts_aten(g, p, C.NUM_CLASSES)
    assert overflow.tolist() == [124 * 123 + 255]
    mapped = vc.map_category_id(g)
    assert int(confusion.sum()) == int((mapped < 124).sum()) - int(((mapped == 123) & (p == 255)).sum())


def test_a_split_line_loses_its_line_ending_only(tmp_path):
    fx = C.load("one_short_of_16")
    submit, data = C.write_tree(fx, str(tmp_path))
    with open(os.path.join(data, fx["split_file"]), "w") as f:
        f.write(fx["split"].rstrip("\n"))                # the reference would look for "v_1" here
    C.check_score(fx, vss.evaluate_vss_files(submit, data, fx["split_file"], device="cpu"))


def test_wrapper_refuses_cpu_tensors():
    x = torch.zeros(9, 4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        vc.vss_video_counts(x, x, 124)
    with pytest.raises(RuntimeError, match="uint8"):
        vc.vss_counts_aten(x.int(), x, 124)


def test_map_category_id():
    raw = torch.tensor([0, 1, 2, 124, 125, 254, 255], dtype=torch.uint8)
    assert vc.map_category_id(raw).tolist() == [255, 0, 1, 123, 124, 253, 255]


def _brute_force(gt, pred, C):
    """The window rule restated pixel by pixel: frame i against each of the next n - 1 frames, on mapped values."""
    T, H, W = gt.shape

    def mapped(v):
        v = 255 if v == 0 else v
        v -= 1
        return 255 if v == 254 else v
    g = [[[mapped(int(gt[t, y, x])) for x in range(W)] for y in range(H)] for t in range(T)]
    windows = np.zeros((T, 2, 2), dtype=np.int64)
    for k, n in enumerate((8, 16)):
        for i in range(T - n + 1):
            for y in range(H):
                for x in range(W):
                    same_g = all(g[i][y][x] == g[i + j][y][x] for j in range(1, n))
                    same_p = all(int(pred[i, y, x]) == int(pred[i + j, y, x]) for j in range(1, n))
                    windows[i, k, 0] += same_g
                    windows[i, k, 1] += same_g and same_p
    confusion = np.zeros((C, C), dtype=np.int64)
    for t in range(T):
        for y in range(H):
            for x in range(W):
                if g[t][y][x] < C:
                    confusion.reshape(-1)[C * g[t][y][x] + int(pred[t, y, x])] += 1
    return confusion, windows


def test_window_rule_against_brute_force():
    rng = np.random.default_rng(0)
    T, H, W, C = 18, 3, 5, 19
    gt = np.repeat(rng.integers(0, 21, (3, H, W)), 6, axis=0).astype(np.uint8)      # runs of six frames ...
    gt[:, 0, :] = 7                                                                 # ... a constant row ...
    gt[:, 1, 0] = np.where(np.arange(T) % 2, 0, 255)                                # ... raw 0 / 255: one label
    gt[9, 2, 3] = 200
    pred = np.repeat(rng.integers(0, 18, (2, H, W)), 9, axis=0).astype(np.uint8)
    pred[:, 0, 0:2] = 3
    pred[5, 0, 1] = 4
    confusion, windows, overflow = vc.vss_counts_aten(torch.from_numpy(gt), torch.from_numpy(pred), C)
    ref_confusion, ref_windows = _brute_force(gt, pred, C)
    assert overflow.tolist() == [-1]
    assert np.array_equal(confusion.numpy(), ref_confusion) and np.array_equal(windows.numpy(), ref_windows)
    assert windows[:11, 0, 0].min() >= W + 1 and windows[0, 1, 0] >= W + 1          # the constant row and the aliased pixel
    assert windows[11:, 0].abs().sum() == 0 and windows[3:, 1].abs().sum() == 0    # windows that do not fit stay zero


def test_the_last_window_that_fits_is_counted_but_not_scored():
    fx = C.load("one_short_of_16")
    v = C.video_counts(fx, "cpu")[0]
    T = len(v.windows)
    assert T == 16 and v.windows[T - 8, 0, 0] > 0 and v.windows[T - 16, 1, 0] > 0   # both windows fit and are counted
    assert len(vss.window_ratios([v], 8)) == T - 8 == len(fx["ratios8"])            # range(T - n): window T - n is left out
    assert len(vss.window_ratios([v], 16)) == 0 == len(fx["ratios16"])              # 16 entries <= 16: the video is skipped
    expected = v.windows[:T - 8, 0, 1] / v.windows[:T - 8, 0, 0]
    assert np.array_equal(np.array(vss.window_ratios([v], 8)), expected)
