"""GPU: the two projections at the head of a deformable-encoder layer in one launch (encoder_ops.linear_pair_blocked,
csrc/linear_pair_f16x3.hip) against the two launches it replaces.

K = 256, A = 256 features in blocks of 32 (value_proj, two passes of 128), B = 288 in blocks of 36 (three passes of 96) or 96 in blocks of
12 (one pass), x [T, S, K], pos [1, S, K]:
  (1, 40)     one ragged tile, less than one workgroup's range
  (3, 301)    the `row % add_rows` wrap falls inside a 32-row tile (rows 301 and 602), ragged tail; with both B's
  (2, 4113)   several workgroups and row ranges

identity  torch.equal with `ops.linear_blocked` on x and on `x + pos.repeat(T, 1)` materialised in torch.  That wrapper answers None below
          64 row tiles (csrc/gemm_plan.h resident_covered), which is every size here but the last: the reference call then carries copies of
          the first batch element behind the T real ones, enough to reach 2048 rows, and its first T elements are compared -- a row's
          result depends on nothing but the row and W, and the blocked layout is per batch element.
          Inputs: gemm_instances.moving_scale_inputs for x, pos and the weights -- rising / falling ramps along k times a power of two per
          row from 2^-30 .. 2^30, so the running row scale is lowered several times inside K, on x in the rows where x is the larger and on
          the sum in the rows where pos is (asserted on the inputs: rows of either kind exist, and in both the block maximum rises by more
          than 2^3 after the first k-step).
  fp64      the family's bounds (tests/test_gemm_instances_gpu.py): plain inputs err < max(4 err32, 5e-6); moving inputs element-wise
          relative to (|x| + |pos|) |w|^T + |b|, e3 < max(4 e32, 3e-7).  The fp64 reference of B sums x and pos in fp64.
  padding   both outputs lie in NaN-filled buffers (256 floats in front and behind): the padding is still NaN afterwards, and no output
          element is NaN (every one was written).
  refusals  K != 256, a B whose passes are not the built kernel's, a misaligned x: None.
  encoder   MSDeformAttnTransformerEncoder, two layers, levels 4 x 6, 8 x 12, 16 x 24: the switch on == the switch off under torch.equal, at
          T = 2 (1008 rows: the standard-layout operators on both sides, below the head-major path's 64 tiles) and at T = 5 (2520 rows: the
          pair kernel runs, once per layer, and the FFN kernel is asked for no `src + pos`).
Every line printed is `EP <T> <S> <N_b> <output> err err32 e3 e32`."""
import pytest
import torch

from tests import gemm_instances as gi
from tests.test_gemm_instances_gpu import PAD, nan_padded_outputs
from univs_amd import encoder_ops, ops
from univs_amd.modeling.pixel_decoder.msdeformattn import MSDeformAttnTransformerEncoder
from univs_amd.switches import override

pytestmark = pytest.mark.gpu
F = torch.nn.functional
K, NA, CA = 256, 256, 32
SHAPES = [(1, 40, 288, 36), (3, 301, 288, 36), (2, 4113, 288, 36), (3, 301, 96, 12)]
_CACHE = {}


def _inputs(T, S, NB, moving, cuda):
    """x [T, S, K], pos [1, S, K], (w, b) of A and B; made once per (shape, kind) and left unchanged"""
    key = (T, S, NB, moving)
    if key not in _CACHE:
        gen = gi.moving_scale_inputs if moving else gi.plain_inputs
        x, wa, ba, _ = gen(T * S, K, NA, f"pair/{NB}")
        pos, wb, bb, _ = gen(S, K, NB, f"pair/pos/{NB}")
        _CACHE[key] = tuple(t.to(cuda) for t in (x.view(T, S, K), pos.view(1, S, K), wa, ba, wb, bb))
        for w in (_CACHE[key][2], _CACHE[key][4]):
            ops.presplit_weights(w)                                            # (cached per tensor: no allocation inside the padded calls)
    return _CACHE[key]


def _pair(t, cb):
    x, pos, wa, ba, wb, bb = t
    with nan_padded_outputs() as made:
        out = encoder_ops.linear_pair_blocked(x, pos, wa, ba, CA, wb, bb, cb)
    assert out is not None, "the pair entry answered None: the case is not covered"
    assert len(made) == 2
    for buf, n in made:
        assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + n:]).all(), "the kernel wrote into the padding around an output"
        assert not torch.isnan(buf[PAD:PAD + n]).any(), "an output element was not written"
    return out


def _blocked_reference(op, w, b, cb):
    """ops.linear_blocked(op [T, S, K]) [T, N / cb, S, cb]; below its 64 row tiles with copies of op[0] behind the T elements (docstring)"""
    T, S, _ = op.shape
    extra = max(0, -(-(2048 - T * S) // S))
    full = torch.cat([op, op[:1].expand(extra, S, K)]).contiguous() if extra else op
    y = ops.linear_blocked(full, w, b, S, cb)
    assert y is not None, "ops.linear_blocked answered None"
    return y[:T]


def _rows(y):
    T, nb, S, cb = y.shape
    return y.permute(0, 2, 1, 3).reshape(T * S, nb * cb)


@pytest.mark.parametrize("T,S,NB,cb", SHAPES)
def test_both_outputs_have_the_bits_of_the_two_launches(cuda, linear_terms, T, S, NB, cb):
    linear_terms(3)
    t = _inputs(T, S, NB, True, cuda)
    x, pos, wa, ba, wb, bb = t
    xq = x + pos.repeat(T, 1, 1)                                               # the materialised operand of B
    # the running scale moves on both kinds of row: block maxima (k-steps of 32) that rise by more than 2^3 after the first k-step
    blocks = xq.view(T * S, K // 32, 32).abs().amax(-1)
    rises = (blocks[:, 1:].amax(-1) > 16 * blocks[:, 0])
    x_larger = (x.abs().amax(-1) > 4 * pos.abs().amax(-1).expand(T, S)).view(-1)
    pos_larger = (pos.abs().amax(-1).expand(T, S) > 4 * x.abs().amax(-1)).reshape(-1)
    assert (rises & x_larger).any() and (rises & pos_larger).any()
    ya, yb = _pair(t, cb)
    ra, rb = _blocked_reference(x, wa, ba, CA), _blocked_reference(xq, wb, bb, cb)
    assert ya.shape == ra.shape and torch.equal(ya, ra), f"A: largest difference {(ya.double() - ra.double()).abs().max().item():.3e}"
    assert yb.shape == rb.shape and torch.equal(yb, rb), f"B: largest difference {(yb.double() - rb.double()).abs().max().item():.3e}"


@pytest.mark.parametrize("T,S,NB,cb", SHAPES)
def test_both_outputs_against_fp64(cuda, linear_terms, T, S, NB, cb):
    linear_terms(3)
    failures = []
    for moving in (False, True):
        t = _inputs(T, S, NB, moving, cuda)
        x, pos, wa, ba, wb, bb = t
        ya, yb = _pair(t, cb)
        x2, p2 = x.view(T * S, K), pos.view(S, K).repeat(T, 1)
        for what, y, w, b, op64, op32, opabs in (("A", ya, wa, ba, x2.double(), x2, x2.double().abs()),
                                                 ("B", yb, wb, bb, x2.double() + p2.double(), x2 + p2, x2.double().abs() + p2.double().abs())):
            ref64 = F.linear(op64, w.double(), b.double())
            d, d32 = (_rows(y).double() - ref64).abs(), (F.linear(op32, w, b).double() - ref64).abs()
            if moving:
                scale = opabs @ w.double().abs().t() + b.double().abs()[None]
                e3, e32 = (d / (scale + 1e-300)).max().item(), (d32 / (scale + 1e-300)).max().item()
                print("EP", T, S, NB, what, "- -", f"{e3:.3e} {e32:.3e}")
                if not e3 < max(4.0 * e32, 3e-7):
                    failures.append(f"{what} moving scale: e3 {e3:.3e} against max(4 x {e32:.3e}, 3e-7)")
            else:
                err, err32 = d.max().item(), d32.max().item()
                print("EP", T, S, NB, what, f"{err:.3e} {err32:.3e}", "- -")
                if not err < max(4.0 * err32, 5e-6):
                    failures.append(f"{what} plain: err {err:.3e} against max(4 x {err32:.3e}, 5e-6)")
    assert not failures, "\n".join(failures)


def test_what_the_entry_does_not_cover_answers_none(cuda, linear_terms):
    linear_terms(3)
    x, pos, wa, ba, wb, bb = _inputs(3, 301, 288, False, cuda)
    g = torch.Generator().manual_seed(7)
    w128 = torch.randn(256, 128, generator=g).to(cuda)
    assert encoder_ops.linear_pair_blocked(x[..., :128].contiguous(), pos[..., :128].contiguous(), w128, ba, CA, w128, ba, CA) is None   # K = 128
    assert encoder_ops.linear_pair_blocked(x, pos, wa, ba, CA, wa, ba, CA) is None             # B = 256: two passes of 128
    assert encoder_ops.linear_pair_blocked(x, pos, wa, ba, CA, wb, bb, 40) is None             # 288 is no multiple of 40
    flat = torch.zeros(x.numel() + 4, device=cuda)
    x_off = flat[1:1 + x.numel()].view(x.shape)                                              # contiguous, 4 bytes off a 16-byte boundary
    assert x_off.is_contiguous() and x_off.data_ptr() % 16 == 4
    assert encoder_ops.linear_pair_blocked(x_off, pos, wa, ba, CA, wb, bb, 36) is None
    with override(resident_presplit=False):                                                    # no split images: the two launches split W themselves
        assert encoder_ops.linear_pair_blocked(x, pos, wa, ba, CA, wb, bb, 36) is None
    assert encoder_ops.linear_pair_blocked(x, pos, wa, ba, CA, wb, bb, 36) is not None


@pytest.mark.parametrize("T,pair_runs", [(2, False), (5, True)])
def test_encoder_is_bit_identical_with_the_switch_on_and_off(cuda, linear_terms, monkeypatch, T, pair_runs):
    linear_terms(3)
    shapes = [(4, 6), (8, 12), (16, 24)]
    starts, S = [0, 24, 120], 504
    torch.manual_seed(11)
    enc = MSDeformAttnTransformerEncoder(256, 1024, 0.0, "relu", 3, 8, 4, 2).to(cuda).eval()
    g = torch.Generator().manual_seed(T)
    src, pos = torch.randn(T, S, 256, generator=g).to(cuda), torch.randn(1, S, 256, generator=g).to(cuda)
    ref = MSDeformAttnTransformerEncoder.get_reference_points(shapes, cuda)
    calls, post_adds = [], []
    real_pair, real_mlp = encoder_ops.linear_pair_blocked, ops.mlp_fused

    def pair(*a, **k):
        out = real_pair(*a, **k)
        calls.append(out is not None)
        return out

    def mlp(*a, **k):
        post_adds.append(k.get("post_add") is not None)
        return real_mlp(*a, **k)
    monkeypatch.setattr(encoder_ops, "linear_pair_blocked", pair)
    monkeypatch.setattr(ops, "mlp_fused", mlp)
    with torch.no_grad():
        with override(encoder_pair=True):
            on = enc(src, shapes, starts, ref, pos, ref_per_query=ref[:, :, 0].contiguous())
            seen_on = (list(calls), list(post_adds))
        calls.clear()
        post_adds.clear()
        with override(encoder_pair=False):
            off = enc(src, shapes, starts, ref, pos, ref_per_query=ref[:, :, 0].contiguous())
    assert not calls                                                          # off: the pair entry is not called
    assert seen_on[0] == ([True, True] if pair_runs else [])                  # on: once per layer where the head-major path applies
    if pair_runs:
        assert not any(seen_on[1])                                            # ... and no `src + pos` asked of the FFN kernel
    assert torch.isfinite(on).all() and torch.equal(on, off)
