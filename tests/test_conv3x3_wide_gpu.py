"""GPU: the 3 x 3 convolution with all 256 output features on one read of x (csrc/conv3x3_wide.hip) behind ops.conv3x3 (x NCHW) and
ops.conv3x3_nhwc (x channels last), against the streamed kernel both entries ran before (csrc/gemm_f16x3_stream.hip, forced through
UnivsConfig.linear_ablate = 12) and against fp64.

Shapes (T, Cin, H, W) at Cout = 256: exactly 4 096 pixels (the smallest M covered, four k-steps per tap); M = 4 150 (no multiple of
the 32-pixel wave tile or of a workgroup round, odd W: image rows wrap inside a wave tile); a frame boundary inside a wave tile (taps
must not leak between frames); three small frames (every border case in one tile column); 73 600 pixels (several rounds per workgroup:
the weight ring runs on across rounds).

Inputs, made once per shape (a row of the GEMM = a pixel, k = tap x Cin + channel):
  plain    tests/gemm_instances.py plain_inputs;
  moving   its moving_scale_inputs (the running row scale is lowered several times along the channels);
  built    `plain` with three pixels whose 32-channel group 1 / 0 / last is scaled by 2^6 -- the outputs around them lower their running
           scale in the middle of a tap, at a tap's first k-step and (the output up-left of the third) at the last k-step of all -- and
           an all-zero pixel;
  broken   `built` with one inf and one nan element: exactly the outputs whose 3 x 3 window contains one of them (same frame) are
           non-finite, and every other output keeps the bits it has for `built`.
Checks: identity (torch.equal between both operand layouts and the streamed kernel under each), fp64 (the bound of
tests/test_ops_gpu.py::test_conv3x3_matches_torch: err < max(4 err32, 1e-5) against F.conv2d in fp64, err32 = F.conv2d in fp32),
padding (every output lies in a NaN-filled buffer: all of y is written and nothing beside it), fallback (Cout = 128 and 16 return what
the streamed kernel returns), run-to-run (two launches are torch.equal).  Every figure is printed before it is asserted: `CW ...`."""
import functools

import pytest
import torch

from tests import gemm_instances as gi
from tests.test_gemm_instances_gpu import PAD, nan_padded_outputs
from univs_amd import ops

pytestmark = pytest.mark.gpu
F = torch.nn.functional
STREAMED = 12                                                     # UnivsConfig.linear_ablate: the entries keep gemm_f16x3_stream
COUT = 256
SHAPES = [(1, 128, 64, 64), (1, 256, 50, 83), (2, 256, 46, 45), (3, 128, 37, 41), (5, 256, 92, 160)]
KINDS = ("plain", "moving", "built", "broken")


def _run(fn, x, w, ablate=0):
    """One launch with its output inside a NaN-filled buffer; the padding must still be NaN afterwards"""
    with ops.configured(linear_ablate=ablate), nan_padded_outputs() as made:
        y = fn(x, w)
    assert y is not None, "not covered"
    assert made, "the wrapper allocated no output through torch.empty"
    for buf, n in made:
        assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + n:]).all(), "a kernel wrote into the padding around its output"
    return y


def _marks(T, Cin, H, W):
    """(pixel (t, y, x), 32-channel group) scaled by 2^6, the zero pixel, the inf and nan elements (t, y, x, channel)"""
    y0, x0 = H // 2, W // 2
    return ([((0, y0, x0 - 8), 1), ((0, y0, x0), 0), ((0, y0, x0 + 8), Cin // 32 - 1)], (T - 1, y0 + 5, x0 - 3), (0, 3, 4, 5),
            (T - 1, H - 2, W - 1, 70))


@functools.lru_cache(maxsize=None)
def _data(shape):
    """Per shape: the four inputs in both layouts, the weight, and the six results of each (2 layouts x {wide, streamed} + a second
    wide launch per layout), all on the GPU"""
    T, Cin, H, W = shape
    dev = torch.device("cuda:0")
    M = T * H * W
    tag = f"conv3x3_wide/{T}x{Cin}x{H}x{W}"
    w = gi.plain_inputs(16, 9 * Cin, COUT, tag + "/w")[1].view(COUT, Cin, 3, 3).to(dev)
    xs = {"plain": gi.plain_inputs(M, Cin, COUT, tag)[0].view(T, H, W, Cin),
          "moving": gi.moving_scale_inputs(M, Cin, COUT, tag)[0].view(T, H, W, Cin)}
    scaled, zero, at_inf, at_nan = _marks(*shape)
    built = xs["plain"].clone()
    for (t, y, x), grp in scaled:
        built[t, y, x, 32 * grp:32 * grp + 32] *= 64.0
    built[zero] = 0.0
    broken = built.clone()
    broken[at_inf] = float("inf")
    broken[at_nan] = float("nan")
    xs.update(built=built, broken=broken)
    out = {"w": w}
    for kind, x in xs.items():
        x_cl = x.to(dev)                                          # [T, H, W, Cin], contiguous: the channels-last operand
        x_nchw = x_cl.permute(0, 3, 1, 2).contiguous()
        out[kind] = {"x": x_nchw,
                     "nchw": _run(ops.conv3x3, x_nchw, w), "nhwc": _run(ops.conv3x3_nhwc, x_cl, w),
                     "nchw_again": _run(ops.conv3x3, x_nchw, w), "nhwc_again": _run(ops.conv3x3_nhwc, x_cl, w),
                     "nchw_streamed": _run(ops.conv3x3, x_nchw, w, STREAMED), "nhwc_streamed": _run(ops.conv3x3_nhwc, x_cl, w, STREAMED)}
    torch.cuda.synchronize()
    return out


def _same(a, b):
    """torch.equal with NaN equal to NaN"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_identity_with_the_streamed_kernel_and_between_layouts(cuda, shape):
    d = _data(shape)
    for kind in KINDS:
        r = d[kind]
        assert tuple(r["nchw"].shape) == (shape[0], COUT, shape[2], shape[3])
        for other in ("nchw_streamed", "nhwc", "nhwc_streamed"):
            diff = (torch.nan_to_num(r["nchw"].double()) - torch.nan_to_num(r[other].double())).abs().max().item()
            print(f"CW identity {shape} {kind} nchw/{other} largest difference {diff:.3e}")
        for other in ("nchw_streamed", "nhwc", "nhwc_streamed"):
            assert _same(r["nchw"], r[other]), (kind, other)
        if kind != "broken":                                     # no NaN: the plain comparison
            assert torch.equal(r["nchw"], r["nchw_streamed"]) and torch.equal(r["nhwc"], r["nhwc_streamed"]) and torch.equal(r["nchw"], r["nhwc"])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_two_launches_agree(cuda, shape):
    d = _data(shape)
    for kind in KINDS:
        assert _same(d[kind]["nchw"], d[kind]["nchw_again"]) and _same(d[kind]["nhwc"], d[kind]["nhwc_again"]), kind


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_matches_fp64(cuda, shape):
    """The bound of test_conv3x3_matches_torch; every element written (an unwritten one is NaN from the padded buffer and fails it)"""
    d = _data(shape)
    fails = []
    for kind in ("plain", "moving", "built"):
        x, w = d[kind]["x"], d["w"]
        ref64 = F.conv2d(x.double(), w.double(), None, 1, 1)
        err32 = (F.conv2d(x, w, None, 1, 1).double() - ref64).abs().max().item()
        for layout in ("nchw", "nhwc"):
            y = d[kind][layout]
            assert not torch.isnan(y).any(), (kind, layout, "an output element was not written")
            err = (y.double() - ref64).abs().max().item()
            print(f"CW fp64 {shape} {kind} {layout} err {err:.3e} err32 {err32:.3e}")
            if not err < max(4.0 * err32, 1e-5):
                fails.append((kind, layout, err, err32))
    assert not fails, fails


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_non_finite_inputs_reach_exactly_their_windows(cuda, shape):
    T, Cin, H, W = shape
    d = _data(shape)
    _, _, at_inf, at_nan = _marks(*shape)
    want = torch.zeros(T, 1, H, W, dtype=torch.bool, device=cuda)
    for t, y, x, _ in (at_inf, at_nan):
        want[t, 0, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    want = want.expand(T, COUT, H, W)
    for layout in ("nchw", "nhwc"):
        got, clean = d["broken"][layout], d["built"][layout]
        assert torch.isfinite(clean).all()
        assert torch.equal(~torch.isfinite(got), want), layout
        assert torch.equal(got[~want], clean[~want]), layout


@pytest.mark.parametrize("cout", [128, 16])
def test_other_feature_counts_keep_the_streamed_kernel(cuda, cout):
    T, Cin, H, W = 1, 256, 50, 83
    tag = f"conv3x3_wide/fallback/{cout}"
    x_cl = gi.moving_scale_inputs(T * H * W, Cin, cout, tag)[0].view(T, H, W, Cin).to(cuda)
    x = x_cl.permute(0, 3, 1, 2).contiguous()
    w = gi.plain_inputs(16, 9 * Cin, cout, tag + "/w")[1].view(cout, Cin, 3, 3).to(cuda)
    for fn, xx in ((ops.conv3x3, x), (ops.conv3x3_nhwc, x_cl)):
        y, ys = _run(fn, xx, w), _run(fn, xx, w, STREAMED)
        assert tuple(y.shape) == (T, cout, H, W) and not torch.isnan(y).any() and torch.equal(y, ys)
