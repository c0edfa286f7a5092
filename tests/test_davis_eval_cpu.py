"""CPU: the ATen formulation of the DAVIS counts and the host arithmetic on them against what the reference recorded (g28 fixtures,
tools/gen_golden_davis_eval.py): the per-frame J / F tables exactly, the returned dictionary with its NaNs, davis-metrics.txt byte for
byte, the error types.  Nothing here reads the reference."""
import os

import numpy as np
import pytest
import torch

from tests import davis_eval_cases as C
from univs_amd.evaluation import davis
from univs_amd.evaluation import davis_counts as dc


@pytest.fixture(scope="module")
def operators():
    fx = C.load("operators")
    return fx, C.operator_counts(fx, dc.davis_counts_aten, "cpu")


def test_operator_cases_equal_the_reference_exactly(operators):
    fx, counts = operators
    assert tuple(fx["radii"].tolist()) == C.RADII and fx["gt"].shape == (3, 64, 96)
    C.check_operators(fx, counts)


def test_operator_counts_are_consistent(operators):
    fx, counts = operators
    g, p = torch.from_numpy(fx["gt"]), torch.from_numpy(fx["pred"])
    for (v, r), (region, n_gt, n_fg, match) in counts.items():
        for i in range(int(fx["G"])):
            area = ((g == i + 1) & ~((g == 255) & bool(v))).sum(dim=(1, 2))
            assert (region[i, :, :, 0].sum(dim=0) <= area).all()
        assert (match[..., 0] <= n_gt[:, None, :]).all() and (match[..., 1] <= n_fg[None, :, :]).all()
    # a larger disk matches no fewer boundary pixels
    for v in (0, 1):
        for a, b in zip(C.RADII[:-1], C.RADII[1:]):
            assert (counts[(v, a)][3] <= counts[(v, b)][3]).all()


@pytest.mark.parametrize("name", C.SCORED)
def test_scene_tables_equal_the_reference_exactly(name):
    C.check_tables(C.load(name), "cpu")


@pytest.mark.parametrize("name", C.SCORED)
def test_evaluate_davis_files_reproduces_dictionary_and_text(name, tmp_path):
    fx = C.load(name)
    root, res = C.write_tree(fx, str(tmp_path))
    out = str(tmp_path / "scores")
    got = davis.evaluate_davis_files(root, res, fx["task"], resolution=fx["resolution"], metrics=fx["metrics"], device="cpu", output_dir=out)
    with open(os.path.join(out, "davis-metrics.txt"), newline="") as f:
        C.check_result(fx, got, f.read())


@pytest.mark.parametrize("name", C.ERRORS)
def test_error_scenes_raise_the_recorded_type(name, tmp_path):
    fx = C.load(name)
    root, res = C.write_tree(fx, str(tmp_path))
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        davis.evaluate_davis_files(root, res, fx["task"], resolution=fx["resolution"], metrics=fx["metrics"], device="cpu")


def test_missing_tree_is_file_not_found(tmp_path):
    with pytest.raises(FileNotFoundError):
        davis.evaluate_davis_files(str(tmp_path / "nowhere"), str(tmp_path), "semi-supervised", device="cpu")
    fx = C.load("semi_clean")
    root, res = C.write_tree(fx, str(tmp_path))
    with pytest.raises(FileNotFoundError):                            # the annotations of the other task are not there
        davis.evaluate_davis_files(root, res, "unsupervised", device="cpu")
    with pytest.raises(FileNotFoundError):                            # a sequence without JPEG images
        davis.evaluate_davis_files(root, res, "semi-supervised", sequences="nobody", device="cpu")


def test_db_statistics_wraps_its_bin_edges_beyond_256_frames():
    fx = C.load("long_300")
    for m, table in (("J", fx["j_long"]), ("F", fx["f_long"])):
        assert table.shape == (2, 298)
        for k in range(2):
            M, R, D = davis.db_statistics(table[k])
            assert C.same([M, R, D], [fx[f"{m}_M"][k], fx[f"{m}_R"][k], fx[f"{m}_D"][k]])
    # below 256 frames the four bins are what they say: the decay of a ramp is the difference of the outer bins' means
    v = np.linspace(1.0, 0.0, 41)
    M, R, D = davis.db_statistics(v)
    assert M == np.mean(v) and R == np.mean(v > 0.5) and D == np.mean(v[0:11]) - np.mean(v[30:41])


def test_disk_radius():
    assert [davis.disk_radius(*s) for s in ((480, 854), (1080, 1920), (2160, 3840), (120, 214), (12, 16))] == [8, 18, 36, 2, 1]
    assert davis.disk_radius(480, 854, bound_th=5) == 5


def test_kernel_wrapper_refuses_cpu_tensors():
    z = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        dc.davis_video_counts(z, z, 1, 1, 1, 0)
    with pytest.raises(RuntimeError, match="uint8"):
        dc.davis_counts_aten(z.int(), z, 1, 1, 1, 0)
    with pytest.raises(RuntimeError, match="radius"):
        dc.davis_counts_aten(z, z, 1, 1, 0, 0)


def test_exports_and_evaluator_name_rules(tmp_path):
    from univs_amd import evaluation
    assert evaluation.evaluate_davis_files is davis.evaluate_davis_files and evaluation.DAVISEvaluator is davis.DAVISEvaluator
    fx = C.load("semi_fewer_results")
    fx["resolution"] = "Full-Resolution"
    root, res = C.write_tree(fx, str(tmp_path))
    out = os.path.dirname(res)
    ev = davis.DAVISEvaluator("davis17_val", os.path.join(root, "JPEGImages", "Full-Resolution"), output_dir=out, device="cpu")
    assert (ev.task, ev.resolution, ev.gt_root) == ("semi-supervised", "Full-Resolution", root)
    ev.reset()
    ev.process([{}], {})
    C.check_result(fx, ev.evaluate())
    with open(os.path.join(out, "davis-metrics.txt"), newline="") as f:
        assert f.read() == str(fx["text"])
    ref = davis.DAVISEvaluator.__new__(davis.DAVISEvaluator)
    with pytest.raises(FileNotFoundError):                            # <root>/DAVIS does not exist
        davis.DAVISEvaluator.__init__(ref, "refdavis_val", os.path.join(root, "JPEGImages", "480p"), output_dir=out)
    with pytest.raises(ValueError):
        davis.DAVISEvaluator("ytvos_val", root, output_dir=out)


def test_command_line(tmp_path, capsys):
    fx = C.load("unsup_clean")
    root, res = C.write_tree(fx, str(tmp_path))
    got = davis.main(["--res_path", res, "--davis_root", root, "--task", "unsupervised", "--device", "cpu", "--output_dir", str(tmp_path)])
    C.check_result(fx, got)
    assert "M:" in capsys.readouterr().out


def test_round_trip_through_the_vos_png_writer(tmp_path):
    """Masks written by the project's own VOS PNG writer (the `inference/Annotations` layout), used as annotation and as result, score
    J = F = 1 on every object."""
    from univs_amd.inference.results import write_vos_pngs
    fx = C.load("semi_clean")
    ids = torch.from_numpy(fx["gt_bear"])
    names = [f"JPEGImages/480p/bear/{n.replace('.png', '.jpg')}" for n in fx["gt_names_bear"].tolist()]
    paths = write_vos_pngs(str(tmp_path / "run"), names, 0, ids)
    res = str(tmp_path / "run" / "inference" / "Annotations")
    assert os.path.dirname(paths[0]) == os.path.join(res, "bear")
    root = str(tmp_path / "DAVIS")                                   # the same PNGs as the annotation side
    write_vos_pngs(str(tmp_path / "gt"), names, 0, ids)
    os.makedirs(os.path.join(root, "Annotations"), exist_ok=True)
    os.rename(str(tmp_path / "gt" / "inference" / "Annotations"), os.path.join(root, "Annotations", "480p"))
    os.makedirs(os.path.join(root, "JPEGImages", "480p", "bear"))
    for n in names:
        open(os.path.join(root, n), "wb").close()
    os.makedirs(os.path.join(root, "ImageSets", "2017"))
    with open(os.path.join(root, "ImageSets", "2017", "val.txt"), "w") as f:
        f.write("bear\n")
    maps, frame_ids = davis.read_sequence(root, "bear", "semi-supervised")
    assert np.array_equal(maps, fx["gt_bear"]) and frame_ids[0] == "00000"
    got = davis.evaluate_davis_files(root, res, "semi-supervised", sequences="bear", device="cpu")
    for m in ("J", "F"):
        assert got[m]["M"] == [1.0, 1.0, 1.0] and got[m]["R"] == [1.0, 1.0, 1.0] and list(got[m]["M_per_object"]) == ["bear_1", "bear_2", "bear_3"]
