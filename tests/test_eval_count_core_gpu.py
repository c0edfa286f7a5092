"""GPU: csrc/count_core.h's hist_add4 through its two users, at the smallest shapes where it can go wrong, against the ATen formulations
(exact).  One row of W = 1067 = 4 * 256 + 43 pixels: a workgroup's first sweep is four full waves, its second one wave of 10 full groups,
one group of 3 pixels and 53 idle lanes, plus three idle waves.  H = 1 is one row segment, so pair_count.hip runs one workgroup per
frame; vss_count.hip runs the two sweeps in two workgroups.  Three maps:

  constant   every full wave holds one cell and takes the shortcut (one lane adds 256); the partial wave must not
  step       constant, but the id changes at pixel 282, inside one lane's four pixels: the two cells hold 282 and 785 per frame
  triples    a new id every 3 pixels: no shortcut anywhere, and the runs straddle the lanes
"""
import numpy as np
import pytest
import torch

from tests import vps_eval_cases as C
from univs_amd.evaluation import pair_counts as pc
from univs_amd.evaluation import vss_counts as vc

pytestmark = pytest.mark.gpu

W, STEP = 1067, 282
MAPS = ["constant", "step", "triples"]


def _index_map(kind, T, n, first):
    """int64 [T, 1, W], indices into a table of n values: `first` (from pixel STEP on: first + 1), or all n in turn"""
    x = np.arange(W)
    row = {"constant": np.full(W, first), "step": first + (x >= STEP), "triples": (x // 3) % n}[kind].astype(np.int64)
    return np.broadcast_to(row, (T, 1, W)).copy()


@pytest.mark.parametrize("enc", ["rgb-rgb", "rgb-i32", "i32-rgb", "i32-i32"])
@pytest.mark.parametrize("kind", MAPS)
def test_pair_counts_one_row(cuda, kind, enc):
    T = 2
    gt_ids = np.array([0, 70000, 131329, 9000000, 16777215], dtype=np.int64)
    pred_ids = np.array([0, 258, 65793, 5000000], dtype=np.int64)
    gt = gt_ids[_index_map(kind, T, len(gt_ids), 1)].astype(np.int32)
    pred = pred_ids[_index_map(kind, T, len(pred_ids), 1)].astype(np.int32)
    ge, pe = enc.split("-")
    g = torch.from_numpy(C.ids_to_rgb(gt) if ge == "rgb" else gt).to(cuda)
    p = torch.from_numpy(C.ids_to_rgb(pred) if pe == "rgb" else pred).to(cuda)
    gi, pi = torch.from_numpy(gt_ids), torch.from_numpy(pred_ids)
    got = pc.panoptic_pair_counts(g, p, gi, pi)
    assert got is not None
    ref = pc.pair_counts_aten(g, p, gi, pi, with_unknown=True)
    assert torch.equal(got[0], ref[0]), (got[0].long() - ref[0].long()).abs().max()
    assert torch.equal(got[1], ref[1]), (got[1], ref[1])
    assert int(got[0].sum()) == T * W
    if kind == "step":
        assert got[0][:, 1, 1].tolist() == [STEP] * T and got[0][:, 2, 2].tolist() == [W - STEP] * T


@pytest.mark.parametrize("kind", MAPS)
def test_vss_video_counts_one_row(cuda, kind):
    T, classes = 9, 19
    gt = (_index_map(kind, T, classes, 4) + 1).astype(np.uint8)           # raw 1 .. 19: mapped 0 .. 18
    pred = _index_map(kind, T, classes, 7).astype(np.uint8)
    g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
    got = vc.vss_video_counts(g, p, classes)
    assert got is not None
    ref = vc.vss_counts_aten(g, p, classes)
    for a, b in zip(got, ref):
        assert torch.equal(a, b), (a.long() - b.long()).abs().max()
    assert int(got[0].sum()) == T * W and int(got[2]) == -1
    if kind == "step":
        assert int(got[0][4, 7]) == T * STEP and int(got[0][5, 8]) == T * (W - STEP)
