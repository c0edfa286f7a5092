"""GPU: csrc/pvos_count.hip against `pvos_counts_aten` (exact) and two closed forms, and the g30 scenes end to end on the device
against what the reference recorded.  Nothing here reads the reference."""
import numpy as np
import pytest
import torch

from tests import pvos_eval_cases as C
from univs_amd.evaluation import pvos_counts as pc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 7, 1, 3, None),             # less than a wave
          (2, 33, 50, 2, 5, None),           # small multi-object case
          (2, 20, 24, 15, 4, None),          # the window is larger than the frame: every pixel is boundary
          (2, 97, 161, 8, 20, None),         # odd plane and tile seams
          (1, 270, 480, 29, 6, None),        # the d of 720 x 1280
          (1, 150, 200, pc.D_MAX, 3, None),  # largest covered d
          (2, 40, 60, 3, 255, 255)]          # every id of a byte, 1 and 255 present


def _both(gt, pred, d, K, cuda):
    g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
    got = pc.pvos_video_counts(g, p, d, K)
    assert got is not None
    ref = pc.pvos_counts_aten(g, p, d, K)
    assert got.dtype == ref.dtype == torch.int32 and got.shape == ref.shape == (gt.shape[0], K, 6)
    for i, n in enumerate(C.CELLS):
        print(n, "sum", int(ref[..., i].sum()), "max |kernel - aten| =", int((got[..., i].long() - ref[..., i].long()).abs().max()))
    assert torch.equal(got, ref)
    return got


@pytest.mark.parametrize("T,H,W,d,K,top", SHAPES)
def test_kernel_equals_aten(cuda, T, H, W, d, K, top):
    gt, pred = C.maps(T, H, W, K, 3 * H + W + d, top)
    got = _both(gt, pred, d, K, cuda)
    for i in (0, 3, 4, 5):                                            # I, BI, B_g, B_p: the equality is not one of zeros
        assert int(got[..., i].sum()) > 0, C.CELLS[i]
    if 2 * d + 1 > max(H, W):
        assert torch.equal(got[..., 3:], got[..., :3])
    if top is not None:
        assert int(got[:, 0, 1].sum()) > 0 and int(got[:, top - 1, 1].sum()) > 0 and int(got[:, top - 1, 5].sum()) > 0


@pytest.mark.parametrize("H,W,d", [(70, 130, 4), (40, 200, 20), (9, 300, 6)])
def test_a_uniform_frame_has_the_frame_of_width_d_as_boundary(cuda, H, W, d):
    m = torch.full((2, H, W), 7, dtype=torch.uint8, device=cuda)
    got = pc.pvos_video_counts(m, m, d, 9)
    ring = H * W - max(0, H - 2 * d) * max(0, W - 2 * d)
    expect = torch.zeros((2, 9, 6), dtype=torch.int32)
    expect[:, 6] = torch.tensor([H * W, H * W, H * W, ring, ring, ring], dtype=torch.int32)
    print("ring", ring, "of", H * W)
    assert torch.equal(got.cpu(), expect)


def test_a_checkerboard_is_all_boundary(cuda):
    H, W = 67, 131
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    m = (1 + (yy + xx) % 2).to(torch.uint8)[None].to(cuda)
    for d in (1, 3):
        got = pc.pvos_video_counts(m, m, d, 2)
        assert torch.equal(got[..., 3:], got[..., :3]) and got[0, :, 1].tolist() == [(H * W + 1) // 2, H * W // 2]


def test_operator_fixture_on_the_device(cuda):
    fx = C.load("operators")
    C.check_operators(fx, C.operator_counts(fx, pc.pvos_video_counts, cuda))


def test_beyond_its_bounds_the_wrapper_answers_none(cuda):
    gt, pred = C.maps(2, 33, 50, 3, 5)
    g, p = torch.from_numpy(gt).to(cuda), torch.from_numpy(pred).to(cuda)
    assert pc.pvos_video_counts(g, p, pc.D_MAX + 1, 3) is None
    got = pc.pvos_counts(g, p, pc.D_MAX + 1, 3)
    assert got.is_cuda and torch.equal(got.cpu(), pc.pvos_counts_aten(g.cpu(), p.cpu(), pc.D_MAX + 1, 3))
    assert pc.pvos_video_counts(g, p, pc.D_MAX, 3) is not None


@pytest.mark.parametrize("name", C.SCORED)
def test_scenes_on_the_device(cuda, name, tmp_path):
    C.check_scene(name, str(tmp_path), cuda)


@pytest.mark.parametrize("name", C.ERRORS)
def test_error_scenes_on_the_device(cuda, name, tmp_path):
    C.check_error_scene(name, str(tmp_path), cuda)


def test_two_calls_on_two_streams_give_equal_results(cuda):
    """A fresh zeroed output and a complete flush per call, whichever stream it runs on."""
    T, H, W, d, K = 2, 97, 161, 8, 20
    g, p = (torch.from_numpy(m).to(cuda) for m in C.maps(T, H, W, K, 11))
    ref = pc.pvos_counts_aten(g, p, d, K)
    torch.cuda.synchronize()
    out = []
    for _ in range(2):
        s = torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(s):
            out.append(pc.pvos_video_counts(g, p, d, K))
        s.synchronize()
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], ref)
