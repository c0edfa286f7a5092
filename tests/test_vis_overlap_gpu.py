"""GPU: csrc/vis_overlap.hip against `vis_overlap_aten` (exact integer equality), and the g29 scene `clean` end to end on the device
against what the reference recorded.  Nothing here reads the reference."""
import numpy as np
import pytest
import torch

from tests import vis_eval_cases as C
from univs_amd import _lib, ops
from univs_amd.evaluation import vis_counts as vc

pytestmark = pytest.mark.gpu


def _both(d_runs, g_runs, T, H, W, cuda):
    """The kernel's table, checked against the ATen formulation on the same device tensors."""
    d_runs, g_runs = d_runs.to(cuda), g_runs.to(cuda)
    got = vc.vis_video_overlap(d_runs, g_runs, T, H, W)
    assert got is not None
    ref = vc.vis_overlap_aten(d_runs, g_runs, T, H, W)
    assert got.dtype == ref.dtype == torch.int32 and got.shape == ref.shape
    print(tuple(got.shape), "sum", int(ref.sum()), "max |kernel - aten| =", int((got.long() - ref.long()).abs().max()))
    assert torch.equal(got, ref)
    return got.cpu()


@pytest.mark.parametrize("D,G,T,H,W", [(5, 3, 3, 37, 53),                # D no multiple of the four waves of a workgroup
                                       (1, 1, 1, 37, 53),
                                       (9, 2, 2, 64, 48)])               # more than one detection per wave
def test_kernel_equals_aten_and_the_dense_count(cuda, D, G, T, H, W):
    d, g = C.blobs(D, T, H, W, 3 * H + D), C.blobs(G, T, H, W, 5 * W + G)
    got = _both(C.runs_of(d), C.runs_of(g), T, H, W, cuda)
    assert torch.equal(got.to(torch.int64), C.brute(d, g)) and int(got.sum()) > 0


def test_combs_against_one_long_run_and_the_reverse(cuda):
    H, W = 37, 53
    long_run = np.zeros(H * W, bool)
    long_run[5:1500] = True
    long_run = long_run.reshape(W, H).T.copy()
    for teeth in (65, 300, 900):                                        # more foreground runs than lanes, than threads, and several rounds
        comb = C.comb(H, W, teeth)
        a, b = C.runs_of(comb[None, None]), C.runs_of(long_run[None, None])
        assert int(a.starts[1]) >= 2 * teeth
        want = int((comb & long_run).sum())
        assert int(_both(a, b, 1, H, W, cuda)) == want > 0
        assert int(_both(b, a, 1, H, W, cuda)) == want


def test_identical_disjoint_and_special_masks_on_each_side(cuda):
    T, H, W = 1, 37, 53
    hw = H * W
    blob = C.blobs(1, 1, H, W, 11)[0, 0]
    lead = blob.copy()
    lead[0, 0] = True                                                   # a leading-foreground mask: the code opens with an empty run
    tail = np.zeros((H, W), bool)
    tail[-1, -1] = tail[-2, -1] = True                                  # foreground touching position H W - 1
    early = np.zeros(hw, bool)
    early[10:400] = True
    late = np.zeros(hw, bool)
    late[400:900] = True                                                # spans that touch and do not meet
    masks = np.stack([blob, lead, np.ones((H, W), bool), np.zeros((H, W), bool), tail, early.reshape(W, H).T, late.reshape(W, H).T, blob])
    runs = C.runs_of(masks[:, None], absent=(7,))                       # the last one absent
    got = _both(runs, runs, T, H, W, cuda)[:, :, 0]
    area = masks.reshape(len(masks), -1).sum(1)
    area[7] = 0
    assert got.diagonal().tolist() == area.tolist()                     # identical masks: the overlap is the area
    assert got[2].tolist() == area.tolist() and got[:, 2].tolist() == area.tolist()      # against the full mask, on either side
    assert got[3].sum() == 0 and got[:, 3].sum() == 0 and got[7].sum() == 0 and got[:, 7].sum() == 0       # empty and absent
    assert got[5, 6] == 0 and got[6, 5] == 0 and got[4, 2] == 2 and got[4, 4] == 2 and got[1, 0] == area[0]


def _gt_of_boundaries(n, H, W):
    """An uncompressed code of exactly n boundaries: n - 1 runs of one pixel and the rest."""
    return {"size": [H, W], "counts": [1] * (n - 1) + [H * W - (n - 1)]}


def test_at_the_lds_tile_it_is_covered_and_one_over_it_is_not(cuda):
    H, W, T = 128, 160, 1
    d = C.runs_of(C.blobs(3, T, H, W, 7))
    for n, covered in ((vc.MAX_BOUNDS - 1, True), (vc.MAX_BOUNDS, True), (vc.MAX_BOUNDS + 1, False)):
        g = vc.runs_from_rles([_gt_of_boundaries(n, H, W), _gt_of_boundaries(12, H, W)], H, W)
        assert int(g.starts[1]) == n
        if covered:
            assert int(_both(d, g, T, H, W, cuda).sum()) > 0
        else:
            assert vc.vis_video_overlap(d.to(cuda), g.to(cuda), T, H, W) is None
            lib = _lib.load()                                           # the entry itself refuses, and says what it covers
            dd, gg = d.to(cuda), g.to(cuda)
            out = torch.zeros((3, 2, 1), dtype=torch.int32, device=cuda)
            rc = lib.univs_vis_overlap_counts(ops._ptr(dd.bounds), ops._ptr(dd.starts), ops._ptr(gg.bounds), ops._ptr(gg.ones), ops._ptr(gg.starts),
                                              3, 2, 1, H, W, n, ops._ptr(out), None)
            assert rc == _lib.ERR_NOT_IMPLEMENTED and "16384 boundaries" in lib.univs_last_error().decode()
            both = vc.vis_overlap(dd, gg, T, H, W)
            assert torch.equal(both, vc.vis_overlap_aten(dd, gg, T, H, W)) and int(both.sum()) > 0


def test_every_cell_is_written_and_a_mask_beyond_the_stated_tile_is_flagged(cuda):
    D, G, T, H, W = 6, 3, 2, 37, 53
    d, g = C.runs_of(C.blobs(D, T, H, W, 21), absent=(3,)).to(cuda), C.runs_of(C.blobs(G, T, H, W, 22), absent=(1,)).to(cuda)
    cap = int(g.starts.diff().max())
    inter = torch.full((D, G, T), -77, dtype=torch.int32, device=cuda)
    args = (ops._ptr(d.bounds), ops._ptr(d.starts), ops._ptr(g.bounds), ops._ptr(g.ones), ops._ptr(g.starts), D, G, T, H, W)
    assert ops._call("test", _lib.load().univs_vis_overlap_counts, inter, *args, cap, ops._ptr(inter))
    assert not bool((inter == -77).any()) and torch.equal(inter, vc.vis_overlap_aten(d, g, T, H, W))
    # a tile stated too small: the masks that do not fit answer -1 in their cells, the others are counted
    inter.fill_(-77)
    assert ops._call("test", _lib.load().univs_vis_overlap_counts, inter, *args, cap - 1, ops._ptr(inter))
    big = (g.starts.diff() == cap).reshape(G, T)
    assert bool(big.any()) and bool((inter[:, big] == -1).all())
    assert torch.equal(inter[:, ~big], vc.vis_overlap_aten(d, g, T, H, W)[:, ~big])


def test_cpu_tensors_raise_the_standard_refusal(cuda):
    d, g = C.runs_of(C.blobs(2, 1, 8, 8, 1)), C.runs_of(C.blobs(2, 1, 8, 8, 2))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        vc.vis_video_overlap(d, g, 1, 8, 8)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        vc.vis_video_overlap(d.to(cuda), g, 1, 8, 8)


def test_clean_scene_on_the_device_equals_the_reference(cuda, monkeypatch):
    calls = []
    kernel = vc.vis_video_overlap

    def counted(*a):
        r = kernel(*a)
        calls.append(r is not None)
        return r
    monkeypatch.setattr(vc, "vis_video_overlap", counted)
    C.check_scene(C.load("clean"), cuda)
    assert calls == [True, True, True]                                  # one kernel call per video, none fell back
