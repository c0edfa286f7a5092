"""GPU: the x-resident form of the encoder layer's two projections (csrc/linear_pair_xres.hip: a wave keeps 16 rows of x and of x + pos as
fp16 parts with their running-scale schedule, the weights stream through LDS in chunks of 32 features) behind the entry of
encoder_ops.linear_pair_blocked, against the W-resident pass kernel it replaces there (csrc/linear_pair_f16x3.hip, forced by
UnivsConfig.linear_ablate = 11) and against the two launches both replace.

K = 256, A = 256 features in blocks of 32, B = 288 in blocks of 36 or 96 in blocks of 12 (the two widths the encoder uses), x [T, S, K],
pos [1, S, K], M = T S rows in groups of 128 (8 waves x 16):
  (1, 1)       the smallest M the entry covers: one row, fifteen of the wave's sixteen repeat it and store nothing
  (1, 127) (1, 128) (1, 129)   one short of, equal to and one past a group; 129: the second group's first wave holds ONE row
  (2, 64)      T = 2: add_rows = M / 2, the wrap on a wave-tile boundary; B = 96
  (3, 43)      T = 3: add_rows = M / 3, the wraps inside wave tiles (rows 43, 86), M = 129
  (3, 91)      M = 273 = 2 x 128 + 17: the last group's second wave holds one row; B = 96
  (3, 11000)   M = 33 000 rows = 258 groups: more groups than any card has CUs, so workgroups walk a second group (the weight
               stream's double buffer runs on across groups)

Inputs, made once per (shape, kind) and left unchanged:
  moving   gemm_instances.moving_scale_inputs as tests/test_encoder_pair_gpu.py: ramps along k times a power of two per row
  built    gemm_instances.plain_inputs with rows BUILT for the schedule, at both ends of M (rows i and M - 1 - i, where M >= 16), so that
           waves hold rows with different schedules -- the lowering is voted wave-wide:
             i = 0  x lowered at k-step 1 only            (columns 32 .. 63 times 2^6)
             i = 1  x lowered at k-step 4 only            (columns 128 .. 159)
             i = 2  x lowered at k-step 7 only, the last  (columns 224 .. 255)
             i = 3  pos lowered at k-step 3 (columns 96 .. 127 times 2^8): x + pos is lowered there, x is not
             i = 4  x all zeros
           asserted on the inputs with the rule of csrc/f16x3_kstep.h replayed in torch (`_lowered_at`).
  nonfinite   `built` with x[5, 70] = inf and x[6, 200] = nan: those two rows are NaN in every feature of both outputs, every other row has
           the bits it has without them.

identity  torch.equal of both outputs with the pass kernel forced, and with `ops.linear_blocked` on x and on x + pos materialised in
          torch (tests/test_encoder_pair_gpu.py: _blocked_reference).
fp64      that file's bound for inputs on which the scale moves, which both kinds here are: element-wise relative to
          (|x| + |pos|) |w|^T + |b|, e3 < max(4 e32, 3e-7) (e32: torch's fp32 Linear).  The fp64 reference of B sums x and pos in fp64.
padding   both outputs lie in NaN-filled buffers: the padding is still NaN, every output element was written.
encoder   MSDeformAttnTransformerEncoder, two layers, levels 4 x 6, 8 x 12, 16 x 24, T = 5 (2520 rows): the new kernel on == off.
Every line printed is `EX <T> <S> <N_b> <kind> <output> err err32 e3 e32`."""
import pytest
import torch

from tests import gemm_instances as gi
from tests.test_encoder_pair_gpu import _blocked_reference, _rows
from tests.test_gemm_instances_gpu import PAD, nan_padded_outputs
from univs_amd import encoder_ops, ops
from univs_amd.modeling.pixel_decoder.msdeformattn import MSDeformAttnTransformerEncoder

pytestmark = pytest.mark.gpu
F = torch.nn.functional
K, NA, CA = 256, 256, 32
OLD_KERNEL = 11                                                                # UnivsConfig.linear_ablate: the entry keeps linear_pair_f16x3
SHAPES = [(1, 1, 288, 36), (1, 127, 288, 36), (1, 128, 288, 36), (1, 129, 288, 36), (2, 64, 96, 12), (3, 43, 288, 36), (3, 91, 96, 12),
          (3, 11000, 288, 36)]
_CACHE = {}


def _lowered_at(op_row):
    """k-steps after the first at which the running scale of f16x3_kstep.h is lowered on one row [K] of an operand"""
    e = torch.frexp(op_row.view(K // 32, 32).abs().amax(-1))[1] - 1            # 2^e <= max < 2^(e+1)
    eset, out = None, []
    for ks, en in enumerate(int(v) for v in e.clamp(-100, 128)):
        if eset is None or en > eset + 2:
            if eset is not None:
                out.append(ks)
            eset = en
    return out


def _built_rows(M):
    return [0, M - 1] if M >= 16 else []


def _inputs(T, S, NB, kind, cuda):
    key = (T, S, NB, kind)
    if key not in _CACHE:
        M = T * S
        gen = gi.moving_scale_inputs if kind == "moving" else gi.plain_inputs
        x, wa, ba, _ = gen(M, K, NA, f"xres/{NB}")
        pos, wb, bb, _ = gen(S, K, NB, f"xres/pos/{NB}")
        if kind != "moving":
            for base in _built_rows(M):
                r = [base + i if base == 0 else base - i for i in range(7)]
                x[r[0], 32:64] *= 64.0
                x[r[1], 128:160] *= 64.0
                x[r[2], 224:256] *= 64.0
                pos[r[3] % S, 96:128] *= 256.0
                x[r[4]] = 0.0
                full = x + pos.repeat(T, 1)
                assert [_lowered_at(x[i]) for i in r[:3]] == [[1], [4], [7]] and [_lowered_at(full[i]) for i in r[:3]] == [[1], [4], [7]]
                assert _lowered_at(x[r[3]]) == [] and _lowered_at(full[r[3]]) == [3]
                if kind == "nonfinite" and base == 0:
                    x[r[5], 70], x[r[6], 200] = float("inf"), float("nan")
        _CACHE[key] = tuple(t.to(cuda) for t in (x.view(T, S, K), pos.view(1, S, K), wa, ba, wb, bb))
        for w in (_CACHE[key][2], _CACHE[key][4]):
            ops.presplit_weights(w)                                            # (cached per tensor: no allocation inside the padded calls)
    return _CACHE[key]


def _pair(t, cb, nan_rows=()):
    x, pos, wa, ba, wb, bb = t
    with nan_padded_outputs() as made:
        out = encoder_ops.linear_pair_blocked(x, pos, wa, ba, CA, wb, bb, cb)
    assert out is not None, "the pair entry answered None: the case is not covered"
    assert len(made) == 2
    for (buf, n), y in zip(made, out):
        assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + n:]).all(), "the kernel wrote into the padding around an output"
        nan = torch.isnan(_rows(y))
        expect = torch.zeros_like(nan)
        if nan_rows:
            expect[list(nan_rows)] = True
        assert torch.equal(nan, expect), "an output element was not written, or a NaN outside the rows that hold one"
    return out


@pytest.mark.parametrize("kind", ["moving", "built"])
@pytest.mark.parametrize("T,S,NB,cb", SHAPES)
def test_both_outputs_have_the_bits_of_the_pass_kernel_and_of_the_two_launches(cuda, linear_terms, T, S, NB, cb, kind):
    linear_terms(3)
    t = _inputs(T, S, NB, kind, cuda)
    x, pos, wa, ba, wb, bb = t
    xq = x + pos.repeat(T, 1, 1)                                               # the materialised operand of B
    ya, yb = _pair(t, cb)
    with ops.configured(linear_ablate=OLD_KERNEL):
        oa, ob = _pair(t, cb)
    ra, rb = _blocked_reference(x, wa, ba, CA), _blocked_reference(xq, wb, bb, cb)
    for what, y, o, r in (("A", ya, oa, ra), ("B", yb, ob, rb)):
        assert y.shape == o.shape == r.shape
        assert torch.equal(y, o), f"{what} against the pass kernel: largest difference {(y.double() - o.double()).abs().max().item():.3e}"
        assert torch.equal(y, r), f"{what} against ops.linear_blocked: largest difference {(y.double() - r.double()).abs().max().item():.3e}"


@pytest.mark.parametrize("T,S,NB,cb", SHAPES)
def test_both_outputs_against_fp64(cuda, linear_terms, T, S, NB, cb):
    linear_terms(3)
    failures = []
    for kind in ("built", "moving"):
        t = _inputs(T, S, NB, kind, cuda)
        x, pos, wa, ba, wb, bb = t
        ya, yb = _pair(t, cb)
        x2, p2 = x.view(T * S, K), pos.view(S, K).repeat(T, 1)
        for what, y, w, b, op64, op32, opabs in (("A", ya, wa, ba, x2.double(), x2, x2.double().abs()),
                                                 ("B", yb, wb, bb, x2.double() + p2.double(), x2 + p2, x2.double().abs() + p2.double().abs())):
            ref64 = F.linear(op64, w.double(), b.double())
            d, d32 = (_rows(y).double() - ref64).abs(), (F.linear(op32, w, b).double() - ref64).abs()
            scale = opabs @ w.double().abs().t() + b.double().abs()[None]
            e3, e32 = (d / (scale + 1e-300)).max().item(), (d32 / (scale + 1e-300)).max().item()
            print("EX", T, S, NB, kind, what, f"{d.max().item():.3e} {d32.max().item():.3e} {e3:.3e} {e32:.3e}")
            if not e3 < max(4.0 * e32, 3e-7):
                failures.append(f"{what} {kind}: e3 {e3:.3e} against max(4 x {e32:.3e}, 3e-7)")
    assert not failures, "\n".join(failures)


def test_inf_and_nan_poison_their_own_rows_only(cuda, linear_terms):
    linear_terms(3)
    T, S, NB, cb = 3, 91, 96, 12
    clean, dirty = _inputs(T, S, NB, "built", cuda), _inputs(T, S, NB, "nonfinite", cuda)
    bad = [5, 6]
    assert torch.isinf(dirty[0].view(-1, K)[5]).any() and torch.isnan(dirty[0].view(-1, K)[6]).any()
    keep = torch.ones(T * S, dtype=torch.bool, device=cuda)
    keep[bad] = False
    want = _pair(clean, cb)
    got = _pair(dirty, cb, nan_rows=bad)                                       # (asserts: NaN in every feature of rows 5 and 6, nowhere else)
    with ops.configured(linear_ablate=OLD_KERNEL):
        old = _pair(dirty, cb, nan_rows=bad)
    for y, o, w in zip(got, old, want):
        assert torch.equal(_rows(y)[keep], _rows(w)[keep]) and torch.equal(_rows(y)[keep], _rows(o)[keep])


def test_encoder_is_bit_identical_with_the_new_kernel_on_and_off(cuda, linear_terms, monkeypatch):
    linear_terms(3)
    T, shapes, starts, S = 5, [(4, 6), (8, 12), (16, 24)], [0, 24, 120], 504
    torch.manual_seed(11)
    enc = MSDeformAttnTransformerEncoder(256, 1024, 0.0, "relu", 3, 8, 4, 2).to(cuda).eval()
    g = torch.Generator().manual_seed(T)
    src, pos = torch.randn(T, S, 256, generator=g).to(cuda), torch.randn(1, S, 256, generator=g).to(cuda)
    ref = MSDeformAttnTransformerEncoder.get_reference_points(shapes, cuda)
    calls, real_pair = [], encoder_ops.linear_pair_blocked

    def pair(*a, **k):
        out = real_pair(*a, **k)
        calls.append(out is not None)
        return out
    monkeypatch.setattr(encoder_ops, "linear_pair_blocked", pair)
    with torch.no_grad():
        on = enc(src, shapes, starts, ref, pos, ref_per_query=ref[:, :, 0].contiguous())
        with ops.configured(linear_ablate=OLD_KERNEL):
            off = enc(src, shapes, starts, ref, pos, ref_per_query=ref[:, :, 0].contiguous())
    assert calls == [True] * 4                                                 # once per layer, on both sides
    assert torch.isfinite(on).all() and torch.equal(on, off)
