"""GPU: csrc/davis_count.hip against `davis_counts_aten` (exact), and the g28 scenes end to end on the device against what the reference
recorded.  Nothing here reads the reference."""
import os

import pytest
import torch

from tests import davis_eval_cases as C
from univs_amd.evaluation import davis
from univs_amd.evaluation import davis_counts as dc

pytestmark = pytest.mark.gpu

NAMES = ("region", "n_gt", "n_fg", "match")
SHAPES = [(3, 5, 7, 1, 1, 1),                # less than a wave
          (2, 33, 50, 2, 3, 5),              # small multi-object case
          (2, 64, 96, 18, 4, 4),             # radius beyond a tile and close to the image
          (2, 97, 161, 8, 5, 20),            # odd plane, so tile edges fall differently in every row
          (1, 480, 854, 8, 3, 3),            # a real row width
          (1, 270, 480, dc.R_MAX, 2, 2),     # largest covered radius
          (2, 40, 60, 5, 32, 32)]            # every bit of the set


def _both(gt, pred, G, P, r, use_void, cuda):
    g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
    got = dc.davis_video_counts(g, p, G, P, r, use_void)
    assert got is not None
    ref = dc.davis_counts_aten(g, p, G, P, r, use_void)
    for name, a, b in zip(NAMES, got, ref):
        assert a.dtype == b.dtype == torch.int32 and a.shape == b.shape, name
        print(name, "use_void", use_void, "sum", int(b.sum()), "max |kernel - aten| =", int((a.long() - b.long()).abs().max()))
        assert torch.equal(a, b), name
    region, n_gt, n_fg, match = got
    for i in range(G):                                               # an object's intersections with disjoint results fit in its area
        area = ((g == i + 1) & ~((g == 255) & bool(use_void))).sum(dim=(1, 2))
        assert (region[i, :, :, 0].sum(dim=0) <= area).all()
    assert (match[..., 0] <= n_gt[:, None, :]).all() and (match[..., 1] <= n_fg[None, :, :]).all()
    return got


@pytest.mark.parametrize("T,H,W,r,G,P", SHAPES)
def test_kernel_equals_aten(cuda, T, H, W, r, G, P):
    gt, pred = C.maps(T, H, W, G, P, 3 * H + W + r)
    for use_void in (0, 1):
        region, n_gt, n_fg, match = _both(gt, pred, G, P, r, use_void, cuda)
        assert int(n_gt.sum()) > 0 and int(n_fg.sum()) > 0 and int(region[..., 1].sum()) > 0
        if T > 1:
            assert int(n_gt[:, T - 1].sum()) == 0                    # the frame without gt objects


def test_operator_fixture_on_the_device(cuda):
    fx = C.load("operators")
    C.check_operators(fx, C.operator_counts(fx, dc.davis_video_counts, cuda))


def test_beyond_its_bounds_the_wrapper_answers_none(cuda):
    T, H, W = 2, 33, 50
    for G, P, r in ((3, 3, dc.R_MAX + 1), (33, 3, 2), (3, 33, 2)):
        gt, pred = C.maps(T, H, W, G, P, 5)
        g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
        assert dc.davis_video_counts(g, p, G, P, r, 1) is None
        got = dc.davis_counts(g, p, G, P, r, 1)
        ref = dc.davis_counts_aten(g.cpu(), p.cpu(), G, P, r, 1)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, ref))
    g, p = (torch.from_numpy(m).to(cuda) for m in C.maps(T, H, W, 3, 3, 5))
    assert dc.davis_video_counts(g, p, 3, 3, dc.R_MAX, 1) is not None


@pytest.mark.parametrize("name", C.SCORED)
def test_scenes_on_the_device(cuda, name, tmp_path):
    fx = C.load(name)
    C.check_tables(fx, cuda)
    root, res = C.write_tree(fx, str(tmp_path))
    out = str(tmp_path / "scores")
    got = davis.evaluate_davis_files(root, res, fx["task"], resolution=fx["resolution"], metrics=fx["metrics"], device=cuda, output_dir=out)
    with open(os.path.join(out, "davis-metrics.txt"), newline="") as f:
        C.check_result(fx, got, f.read())


@pytest.mark.parametrize("name", C.ERRORS)
def test_error_scenes_on_the_device(cuda, name, tmp_path):
    fx = C.load(name)
    root, res = C.write_tree(fx, str(tmp_path))
    with pytest.raises(C.ERROR_TYPES[str(fx["error"])]):
        davis.evaluate_davis_files(root, res, fx["task"], resolution=fx["resolution"], metrics=fx["metrics"], device=cuda)


def test_two_calls_on_two_streams_give_equal_results(cuda):
    """Fresh zeroed outputs and a complete flush per call, whichever stream it runs on."""
    T, H, W, r, G, P = 2, 97, 161, 8, 5, 20
    g, p = (torch.from_numpy(m).to(cuda) for m in C.maps(T, H, W, G, P, 11))
    ref = dc.davis_counts_aten(g, p, G, P, r, 1)
    torch.cuda.synchronize()
    out = []
    for _ in range(2):
        s = torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(s):
            out.append(dc.davis_video_counts(g, p, G, P, r, 1))
        s.synchronize()
    for a, b, c in zip(out[0], out[1], ref):
        assert torch.equal(a, b) and torch.equal(a, c)
