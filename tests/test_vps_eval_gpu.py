"""GPU: csrc/pair_count.hip against `pair_counts_aten` (exact), and the g26 scenes end to end on the device against what the
reference recorded.  Nothing here reads the reference."""
import numpy as np
import pytest
import torch

from tests import vps_eval_cases as C
from univs_amd.evaluation import pair_counts as pc
from univs_amd.evaluation import vps

pytestmark = pytest.mark.gpu


def _ids(n, seed):
    """n ascending ids, VOID first, all three bytes non-zero beyond it."""
    rng = np.random.default_rng(seed)
    ids = set()
    while len(ids) < n - 1:
        r, g, b = rng.integers(1, 256, 3)
        ids.add(int(r) + 256 * int(g) + 65536 * int(b))
    return np.array([0] + sorted(ids), dtype=np.int64)


def _runs(T, H, W, ids, seed, run=37):
    """An id map of runs (panoptic maps are runs) with some single-pixel noise."""
    rng = np.random.default_rng(seed)
    n = T * H * W
    base = np.repeat(rng.integers(0, len(ids), n // run + 1), run)[:n]
    noise = rng.random(n) < 0.02
    base[noise] = rng.integers(0, len(ids), int(noise.sum()))
    return ids[base].reshape(T, H, W).astype(np.int32)


def _both(gt, pred, gt_ids, pred_ids, cuda):
    g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
    gi, pi = torch.from_numpy(gt_ids), torch.from_numpy(pred_ids)
    got = pc.panoptic_pair_counts(g, p, gi, pi)
    assert got is not None
    ref = pc.pair_counts_aten(g, p, gi, pi, with_unknown=True)
    assert torch.equal(got[0], ref[0]), (got[0].long() - ref[0].long()).abs().max()
    assert torch.equal(got[1], ref[1]), (got[1], ref[1])
    assert int(got[0].sum()) == gt.shape[0] * gt.shape[1] * gt.shape[2]
    return got


@pytest.mark.parametrize("T,H,W,G,P", [(1, 97, 161, 40, 40), (12, 97, 161, 40, 2), (1, 720, 1280, 40, 40), (12, 33, 50, 1, 1),
                                       (2, 64, 96, 127, 127), (3, 31, 3, 2, 40)])
@pytest.mark.parametrize("enc", ["rgb-rgb", "rgb-i32", "i32-rgb", "i32-i32"])
def test_kernel_equals_aten(cuda, T, H, W, G, P, enc):
    gt_ids, pred_ids = _ids(G, 1), _ids(P, 2)
    gt, pred = _runs(T, H, W, gt_ids, 3), _runs(T, H, W, pred_ids, 4, run=53)
    ge, pe = enc.split("-")
    _both(C.ids_to_rgb(gt) if ge == "rgb" else gt, C.ids_to_rgb(pred) if pe == "rgb" else pred, gt_ids, pred_ids, cuda)


def test_unknown_ids_fill_the_bucket_and_are_named(cuda):
    gt_ids, pred_ids = _ids(10, 5), _ids(12, 6)
    gt, pred = _runs(4, 97, 161, gt_ids, 7), _runs(4, 97, 161, pred_ids, 8)
    gt[1, 10:20, 30:60] = 0x030201                       # not listed
    gt[1, 50, 5] = 0x050403
    pred[3, 0:7, 100:161] = 0x7F0102
    for g, p in ((C.ids_to_rgb(gt), C.ids_to_rgb(pred)), (gt, pred)):
        counts, unknown = _both(g, p, gt_ids, pred_ids, cuda)
        assert int(counts[1, 10].sum()) == 301 and int(counts[3, :, 12].sum()) == 7 * 61
        assert unknown.tolist() == [[-1, -1], [0x050403, -1], [-1, -1], [-1, 0x7F0102]]


def test_all_void_frame(cuda):
    gt_ids, pred_ids = _ids(40, 9), _ids(40, 10)
    gt, pred = _runs(3, 97, 161, gt_ids, 11), _runs(3, 97, 161, pred_ids, 12)
    gt[1], pred[1] = 0, 0
    counts, _ = _both(C.ids_to_rgb(gt), C.ids_to_rgb(pred), gt_ids, pred_ids, cuda)
    assert int(counts[1, 0, 0]) == 97 * 161 and int(counts[1].sum()) == 97 * 161


def test_beyond_the_lds_bound_the_wrapper_answers_none(cuda):
    gt_ids, pred_ids = _ids(200, 13), _ids(200, 14)
    gt, pred = _runs(2, 97, 161, gt_ids, 15), _runs(2, 97, 161, pred_ids, 16)
    g, p = torch.from_numpy(C.ids_to_rgb(gt)).to(cuda), torch.from_numpy(pred).to(cuda)
    gi, pi = torch.from_numpy(gt_ids), torch.from_numpy(pred_ids)
    assert pc.panoptic_pair_counts(g, p, gi, pi) is None
    counts, unknown = pc.pair_counts(g, p, gi, pi)
    ref = pc.pair_counts_aten(g.cpu(), p.cpu(), gi, pi)
    assert torch.equal(counts.cpu(), ref) and int(unknown.max()) == -1


@pytest.mark.parametrize("name", C.SCORED)
def test_scores_from_tables_on_the_device(cuda, name):
    fx = C.load(name)
    C.check_score(fx, vps.score_tables(C.tables(fx, cuda), fx["gt_json"]))


@pytest.mark.parametrize("name", ["clean", "crowd_void"])
def test_evaluate_vps_files_on_the_device(cuda, name, tmp_path):
    fx = C.load(name)
    submit, truth, gt_file = C.write_tree(fx, str(tmp_path))
    C.check_score(fx, vps.evaluate_vps_files(submit, truth, gt_file, device=cuda))
    C.check_files(fx, submit)


@pytest.mark.parametrize("name", C.ERRORS[:4])
def test_error_scenes_on_the_device(cuda, name, tmp_path):
    fx = C.load(name)
    submit, truth, gt_file = C.write_tree(fx, str(tmp_path))
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        vps.evaluate_vps_files(submit, truth, gt_file, device=cuda)


def test_evaluator_on_the_device(cuda, tmp_path):
    fx = C.load("clean")
    score, out_dir, truth, gt_file, _ = C.run_evaluator(fx, str(tmp_path), cuda)
    files = vps.evaluate_vps_files(out_dir, truth, gt_file, device=cuda, output_dir=str(tmp_path / "again"))
    assert score["files"] == files["files"]
