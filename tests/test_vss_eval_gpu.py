"""GPU: csrc/vss_count.hip against `vss_counts_aten` (exact), and the g27 scenes end to end on the device against what the reference
recorded.  Nothing here reads the reference."""
import os

import numpy as np
import pytest
import torch

from tests import vss_eval_cases as C
from univs_amd.evaluation import vss
from univs_amd.evaluation import vss_counts as vc

pytestmark = pytest.mark.gpu

SHAPES = [(9, 5, 7),          # H W odd, less than one wave
          (17, 97, 161),      # an odd plane: every frame is misaligned differently
          (8, 33, 50),        # no VC8 window is scored, one fits
          (16, 33, 50),       # the same for VC16
          (40, 64, 96),
          (3, 480, 853)]      # a real row width


def _runs(T, H, W, values, seed, run=37, hold=5):
    """A uint8 map of runs in space (`run` pixels) and time (`hold` frames) over `values`, with 2 % single-pixel noise."""
    rng = np.random.default_rng(seed)
    n = H * W
    keys = (T + hold - 1) // hold
    base = np.repeat(rng.integers(0, len(values), (keys, n // run + 1)), run, axis=1)[:, :n]
    base = np.repeat(base, hold, axis=0)[:T].copy()
    noise = rng.random((T, n)) < 0.02
    base[noise] = rng.integers(0, len(values), int(noise.sum()))
    return np.asarray(values, dtype=np.uint8)[base].reshape(T, H, W)


def _maps(T, H, W, num_classes, seed):
    """Raw gt over 0, 255, the classes and a few values in 125..254; predictions below num_classes; rows with the special cases."""
    gt_values = [0, 255] + list(range(1, min(num_classes, 124) + 1)) + [125, 200, 254]
    gt = _runs(T, H, W, gt_values, seed)
    pred = _runs(T, H, W, list(range(num_classes)), seed + 1, run=53, hold=7)
    t = np.arange(T)
    gt[:, 0, :] = np.where(t % 2, 0, 255)[:, None]                   # raw 0 / 255 alternate: one label after the map
    gt[:, 1, :] = 3                                                  # constant on both sides: common in every window
    pred[:, 1, :] = 2
    gt[:, 2, :] = (1 + t % 5)[:, None]                               # changes everywhere every frame
    gt[:, H - 1, W // 2:] = 130 + (t // 9)[:, None]                  # 125..254: outside mIoU, inside VC
    return gt, pred


def _both(gt, pred, num_classes, cuda):
    g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
    got = vc.vss_video_counts(g, p, num_classes)
    assert got is not None
    ref = vc.vss_counts_aten(g, p, num_classes)
    for name, a, b in zip(("confusion", "windows", "overflow"), got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        print(name, "max |kernel - aten| =", int((a.long() - b.long()).abs().max()))
        assert torch.equal(a, b), name
    mapped = vc.map_category_id(g)
    if int(got[2]) < 0:
        assert int(got[0].sum()) == int((mapped < num_classes).sum())
    return got


@pytest.mark.parametrize("T,H,W", SHAPES)
@pytest.mark.parametrize("num_classes", [124, 19])
def test_kernel_equals_aten(cuda, T, H, W, num_classes):
    gt, pred = _maps(T, H, W, num_classes, 7 * T + H)
    confusion, windows, overflow = _both(gt, pred, num_classes, cuda)
    assert int(overflow) == -1
    for k, n in enumerate((8, 16)):
        if T >= n:
            assert int(windows[:T - n + 1, k, 0].min()) >= 2 * W    # the aliased row and the constant row
            assert int(windows[:T - n + 1, k, 1].min()) >= W
        assert int(windows[max(0, T - n + 1):, k].abs().sum()) == 0


def test_kernel_equals_aten_at_the_lds_bound(cuda):
    gt, pred = _maps(17, 97, 161, 128, 3)
    gt[4, 10:12, 5:30] = 128                                         # mapped 127, the last row
    pred[4, 10:20, 5:60] = 255                                       # later rows of the flattened matrix, and beyond it
    _, _, overflow = _both(gt, pred, 128, cuda)
    assert int(overflow) >= 128 * 128


def test_constant_and_all_changing_videos(cuda):
    T, H, W = 20, 33, 50
    gt = np.full((T, H, W), 9, np.uint8)
    pred = np.full((T, H, W), 8, np.uint8)
    _, windows, _ = _both(gt, pred, 124, cuda)
    assert windows[:T - 7, 0].eq(H * W).all() and windows[:T - 15, 1].eq(H * W).all()
    gt = (1 + (np.arange(T)[:, None, None] + np.arange(H * W).reshape(1, H, W)) % 100).astype(np.uint8)
    confusion, windows, _ = _both(gt, pred, 124, cuda)
    assert int(windows.abs().sum()) == 0 and int(confusion.sum()) == T * H * W


def test_overflow_flag_equals_aten(cuda):
    gt, pred = _maps(9, 33, 50, 124, 11)
    gt[5, 4:8, :] = 124                                              # mapped 123 ...
    pred[5, 4:8, 10:20] = 255                                        # ... under 255: cell 124 * 123 + 255
    gt[6, 9, :] = 123
    pred[6, 9, 3] = 250
    _, _, overflow = _both(gt, pred, 124, cuda)
    assert overflow.tolist() == [124 * 123 + 255]
    with pytest.raises(ValueError):
        vss._count(gt, pred, 124, cuda)


def test_beyond_the_lds_bound_the_wrapper_answers_none(cuda):
    gt, pred = _maps(9, 33, 50, 150, 13)
    g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
    assert vc.vss_video_counts(g, p, 150) is None
    got = vc.vss_counts(g, p, 150)
    ref = vc.vss_counts_aten(g.cpu(), p.cpu(), 150)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, ref))


@pytest.mark.parametrize("name", C.SCORED)
def test_scores_from_counts_on_the_device(cuda, name):
    fx = C.load(name)
    C.check_score(fx, vss.score_counts(C.video_counts(fx, cuda), fx["split_file"]))


@pytest.mark.parametrize("name", C.SCORED)
def test_evaluate_vss_files_on_the_device(cuda, name, tmp_path):
    fx = C.load(name)
    submit, data = C.write_tree(fx, str(tmp_path))
    C.check_score(fx, vss.evaluate_vss_files(submit, data, fx["split_file"], device=cuda))
    C.check_files(fx, submit)


@pytest.mark.parametrize("name", C.ERRORS)
def test_error_scenes_on_the_device(cuda, name, tmp_path):
    fx = C.load(name)
    submit, data = C.write_tree(fx, str(tmp_path))
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        vss.evaluate_vss_files(submit, data, fx["split_file"], device=cuda)


def test_a_workgroup_walks_more_than_one_tile(cuda):
    """1025 x 1031 pixels are 1033 tiles of 1024 positions for at most 1024 workgroups: some workgroups take a second tile, with
    fresh run lengths and the same window records."""
    T, H, W = 9, 1025, 1031
    gt, pred = _maps(T, H, W, 124, 5)
    gt[6, H - 1, W - 40:] = 124                                      # an overflowing cell in the last tile: the flag survives the stride
    pred[6, H - 1, W - 40:] = 255
    _, windows, overflow = _both(gt, pred, 124, cuda)
    assert int(windows[0, 0, 0]) >= 2 * W and int(windows[1, 0, 0]) >= 2 * W and overflow.tolist() == [124 * 123 + 255]


def test_a_misaligned_map_is_not_covered(cuda):
    T, H, W = 9, 33, 50
    gt, pred = _maps(T, H, W, 124, 17)
    store = torch.zeros(T * H * W + 8, dtype=torch.uint8, device=cuda)
    store[1:1 + T * H * W] = torch.from_numpy(gt).to(cuda).reshape(-1)
    g = store[1:1 + T * H * W].view(T, H, W)                         # contiguous, one byte off a dword
    p = torch.from_numpy(pred).to(cuda)
    assert g.data_ptr() % 4 == 1 and g.is_contiguous()
    ref = vc.vss_counts_aten(torch.from_numpy(gt), torch.from_numpy(pred), 124)
    for a, b in ((g, p), (p, g)):
        assert vc.vss_video_counts(a, b, 124) is None
    assert all(torch.equal(x.cpu(), y) for x, y in zip(vc.vss_counts(g, p, 124), ref))


def test_beyond_the_frame_bound_the_wrapper_answers_none(cuda):
    T, H, W = 1025, 4, 5
    gt, pred = _maps(T, H, W, 19, 19)
    g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
    assert vc.vss_video_counts(g, p, 19) is None
    assert vc.vss_video_counts(g[:1024].contiguous(), p[:1024].contiguous(), 19) is not None
    ref = vc.vss_counts_aten(torch.from_numpy(gt), torch.from_numpy(pred), 19)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(vc.vss_counts(g, p, 19), ref))


@pytest.mark.parametrize("name", C.ERRORS)
def test_evaluator_raises_the_error_scenes_on_the_device(cuda, name, tmp_path):
    fx = C.load(name)
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        C.run_evaluator(fx, str(tmp_path), cuda)


@pytest.mark.parametrize("name", C.EVALUATOR_SCORED)
def test_evaluator_on_the_device(cuda, name, tmp_path, monkeypatch):
    fx = C.load(name)
    score, submit, data, opened = C.run_evaluator(fx, str(tmp_path), cuda, monkeypatch)
    C.check_score(fx, score)
    C.check_files(fx, os.path.dirname(submit))
    assert opened == []
    files = vss.evaluate_vss_files(submit, data, fx["split_file"], device=cuda, output_dir=str(tmp_path / "again"))
    assert score["files"] == files["files"]
