"""GPU: the decoder's few-rows kernels (csrc/small_linear.hip: small_linear_kernel<false>, small_chain_kernel; csrc/proca_attn.hip) at
their tile edges and over wide row ranges, against fp64 (tests/small_rows_cases.py: the cases, the families and the path each case is
there for; tests/test_small_rows_family_cpu.py pins the table to the paths and the bound to the arithmetic).

small_linear / small_mlp, per case and family:
  error     ref64 = the wrapper's expression in fp64 from the device tensors (x + x_add formed in fp64); element-wise relative to
            scale = |x + x_add| |W[rows]|^T + |b[rows]| + |residual|: e3 < max(4 e32, 3e-7), e32 = the fp32 expression against the same
            reference -- the bound of tests/test_gemm_instances_gpu.py unchanged: the factor is the family's own, the floor the
            per-product bound 2^-21.7 of linear_f16x3.hip (the numpy restatement stays below 1.2e-7 on these inputs).  The LayerNorm
            epilogue: against fp64 F.layer_norm of ref64, relative to max(1, |ref|), floor 2e-6 (test_small_linear_norm_conditioning).
  siblings  bit for bit: the two sides of an `add_features` launch against the launches of each side alone, the transposed store
            against the plain one, the chain against the chain of small_linear launches (with the input LayerNorm: on its returned rows).
  stages    every stage of a chain as a small_linear launch on the GPU output of the stage before, against one fp64 Linear of that
            same input: every hand-over is judged at its own scale.
  padding   every output lies in a NaN-filled buffer; the padding is still NaN afterwards, an unwritten element fails the bound as NaN.
  bad rows  a NaN or an Inf in one row of a 16-row tile (mid-tile, and the last row, which the rows past M repeat): every other row
            keeps the bits of the clean run.
proca_attention: e = |out - ref64| relative to sum_l p_l |v_l| per element, e < max(4 e32, 2e-5) (the absolute figure of
test_proca_attention_matches_the_reference_sequence, whose unit-normal case has a scale of order 1).
Every line printed is `SR <case> <family> e3 e32` or `PA <case> <family> e e32` (profiles/small_rows_family_v1.txt).

What the file sees, tried once on a deliberately wrong build: with the row maxima of small_linear_kernel shared by pairs of rows
(`rmax[.][j_ & ~1]`) and proca's softmax without the subtraction of the maximum, 28 of the 31 tests here fail (e3 up to 0.7; NaN on
`sharp` and `offset`) while every older small_linear / small_mlp / proca test of tests/test_ops_gpu.py, test_norm_conditioning_gpu.py
and test_seam_fold_gpu.py still passes."""
import pytest
import torch

from tests import small_rows_cases as sr
from tests.test_gemm_instances_gpu import PAD, nan_padded_outputs
from tests.test_norm_conditioning_gpu import within
from univs_amd import ops

pytestmark = pytest.mark.gpu
F = torch.nn.functional
LN_EPS = 1e-5
SL_LN_FLOOR = 2e-6          # test_small_linear_norm_conditioning: the floor of this epilogue
CHAIN_LN_FLOOR = 2e-5       # tests/test_norm_conditioning_gpu.py LN_FLOOR: a LayerNorm's own output


def padded(fn):
    """fn() with its outputs NaN-padded; never None"""
    with nan_padded_outputs() as made:
        y = fn()
    assert y is not None, "the wrapper answered None: the case is not covered"
    assert made, "the wrapper allocated no output through torch.empty"
    for buf, n in made:
        assert torch.isnan(buf[:PAD]).all() and torch.isnan(buf[PAD + n:]).all(), "a kernel wrote into the padding around its output"
    return y


def bound(e3, e32):
    return e3 < max(4.0 * e32, 3e-7)


def rel_err(y, ref64, scale):
    return ((y.double() - ref64).abs() / (scale + 1e-300)).max().item()         # (NaN if y holds one: fails every bound)


def _dev(t, cuda):
    return {k: (v.to(cuda) if v is not None else None) for k, v in t.items()}


# ---- small_linear ------------------------------------------------------------------------------------------------------------------------
def sl(c, t, x=None, xa=None, transposed=None):
    """The case's launch -> rows [M, N]"""
    M, K, T = c["M"], c["K"], c["out_T"] if transposed is None else transposed
    x, xa = (t["x"] if x is None else x), (t["xa"] if xa is None else xa)
    shape = (M // T, T, K) if T else (M, K)
    y = padded(lambda: ops.small_linear(x.view(shape), t["w"], t["b"], rows=c["rows"], x_add=xa.view(shape) if xa is not None else None,
                                        relu=c["relu"], residual=t["r"], ln=(t["g"], t["be"], LN_EPS) if c["ln"] else None,
                                        add_features=c["add_features"], transpose01=bool(T)))
    N = sr.feature_range(c)[1]
    if T:
        assert tuple(y.shape) == (T, M // T, N) and y.is_contiguous()
        return y.permute(1, 0, 2).reshape(M, N)
    assert tuple(y.shape) == (M, N)
    return y


def sl_refs(c, t):
    """(ref(dtype) without the LayerNorm, scale)"""
    f_off, N = sr.feature_range(c)
    af = c["add_features"]

    def sides(dt, mag=False):
        v = (lambda a: a.to(dt).abs()) if mag else (lambda a: a.to(dt))
        w = v(t["w"])[f_off:f_off + N]
        xs = t["x"].to(dt) + t["xa"].to(dt) if t["xa"] is not None else t["x"].to(dt)
        xs = xs.abs() if mag else xs
        if af:
            return [(xs, w[:af], slice(0, af)), (v(t["x"]), w[af:], slice(af, N))]
        return [(xs, w, slice(0, N))]

    def ref(dt):
        b = t["b"].to(dt)[f_off:f_off + N]
        y = torch.cat([F.linear(xo, w, b[s]) for xo, w, s in sides(dt)], -1)
        y = y.relu() if c["relu"] else y
        return y + t["r"].to(dt) if t["r"] is not None else y
    scale = torch.cat([xo @ w.t() for xo, w, _ in sides(torch.float64, True)], -1) + t["b"].double().abs()[f_off:f_off + N][None]
    if t["r"] is not None:
        scale = scale + t["r"].double().abs()
    return ref, scale


def sl_siblings(c, t, y):
    """(what, rows of y, the sibling's result)"""
    f_off, N = sr.feature_range(c)
    af = c["add_features"]
    if af:
        r_lo, r_hi = (None, None) if t["r"] is None else (t["r"][:, :af].contiguous(), t["r"][:, af:].contiguous())
        lo = padded(lambda: ops.small_linear(t["x"], t["w"], t["b"], rows=(f_off, af), x_add=t["xa"], relu=c["relu"], residual=r_lo))
        hi = padded(lambda: ops.small_linear(t["x"], t["w"], t["b"], rows=(f_off + af, N - af), relu=c["relu"], residual=r_hi))
        yield "the launch of the x + x_add features alone", y[:, :af], lo
        yield "the launch of the plain features alone (no x_add)", y[:, af:], hi
    if c["out_T"]:
        yield "the untransposed result, permuted", y, sl(c, t, transposed=0)


@pytest.mark.parametrize("c", sr.SL_CASES, ids=lambda c: c["id"])
def test_small_linear_family_against_fp64(cuda, c):
    failures = []
    for fam in sr.families_of(c):
        t = _dev(sr.sl_inputs(c, fam), cuda)
        y = sl(c, t)
        ref, scale = sl_refs(c, t)
        ref64, ref32 = ref(torch.float64), ref(torch.float32)
        if c["ln"]:
            N = y.shape[1]
            ln64 = F.layer_norm(ref64, (N,), t["g"].double(), t["be"].double(), LN_EPS)
            ln32 = F.layer_norm(ref32, (N,), t["g"], t["be"], LN_EPS)
            s = max(1.0, ln64.abs().max().item())
            e3, e32 = (y.double() - ln64).abs().max().item() / s, (ln32.double() - ln64).abs().max().item() / s
            print("SR", c["id"], fam, f"{e3:.3e} {e32:.3e}")
            if not within(e3, e32, SL_LN_FLOOR):
                failures.append(f"{fam}: LayerNorm epilogue {e3:.3e} against max(4 x {e32:.3e}, {SL_LN_FLOOR})")
        else:
            e3, e32 = rel_err(y, ref64, scale), rel_err(ref32, ref64, scale)
            print("SR", c["id"], fam, f"{e3:.3e} {e32:.3e}")
            if not bound(e3, e32):
                failures.append(f"{fam}: e3 {e3:.3e} against max(4 x {e32:.3e}, 3e-7)")
        for what, mine, other in sl_siblings(c, t, y):
            if not (other.shape == mine.shape and torch.equal(other, mine)):
                failures.append(f"{fam}: not the bits of {what} (largest difference {(other.double() - mine.double()).abs().max().item():.3e})")
    assert not failures, c["id"] + ":\n  " + "\n  ".join(failures)


def _bad_rows(M):
    return (16 * (M // 32) + 8, M - 1)          # the middle of a tile; the row that the rows past M repeat


def _others_equal(y, clean, r):
    keep = torch.arange(y.shape[0], device=y.device) != r
    return torch.equal(y[keep], clean[keep])


@pytest.mark.parametrize("cid", sr.SL_BAD_ROW_CASES)
def test_small_linear_bad_row_stays_in_its_row(cuda, cid):
    c = sr.SL_BY_ID[cid]
    t = _dev(sr.sl_inputs(c, "rows"), cuda)
    clean = sl(c, t)
    assert torch.isfinite(clean).all()
    col = c["K"] // 2 + 5
    af = c["add_features"]
    for r in _bad_rows(c["M"]):
        assert r != 3                               # (the zero row of the family)
        for bad in (float("nan"), float("inf")):
            x = t["x"].clone()
            x[r, col] = bad
            y = sl(c, t, x=x)
            assert _others_equal(y, clean, r), (cid, r, bad, "another row changed")
            assert torch.isnan(y[r]).all() if bad != bad else not torch.isfinite(y[r]).any(), (cid, r, bad, y[r])
        if af:
            xa = t["xa"].clone()
            xa[r, col] = float("nan")
            y = sl(c, t, xa=xa)
            assert _others_equal(y, clean, r), (cid, r, "x_add: another row changed")
            assert torch.equal(y[r, af:], clean[r, af:]) and torch.isnan(y[r, :af]).all(), (cid, r, "x_add")


# ---- small_mlp ---------------------------------------------------------------------------------------------------------------------------
def _chain_dev(M, stages, fam, cuda):
    x, lay = sr.chain_inputs(M, stages, fam)
    return x.to(cuda), [(w.to(cuda), b.to(cuda) if b is not None else None, relu) for w, b, relu in lay]


def _ln_params(cuda):
    g = torch.Generator().manual_seed(256)
    return (1.0 + 0.3 * torch.randn(256, generator=g)).to(cuda), (0.2 * torch.randn(256, generator=g)).to(cuda)


@pytest.mark.parametrize("in_ln", (False, True), ids=("plain", "in_ln"))
@pytest.mark.parametrize("stages", sr.CHAIN_STAGES)
@pytest.mark.parametrize("M", sr.CHAIN_M)
def test_small_mlp_chain_stage_by_stage(cuda, M, stages, in_ln):
    failures = []
    name = f"chain_m{M}_s{stages}" + ("_ln" if in_ln else "")
    for fam in sr.CHAIN_FAMILIES:
        x, lay = _chain_dev(M, stages, fam, cuda)
        if in_ln:
            g_, b_ = _ln_params(cuda)
            got, h = padded(lambda: ops.small_mlp(x, lay, in_ln=(g_, b_, LN_EPS), want_normed=True))
            again = padded(lambda: ops.small_mlp(x, lay, in_ln=(g_, b_, LN_EPS)))
            if not torch.equal(again, got):
                failures.append(f"{fam}: the output changes with want_normed")
            n64 = F.layer_norm(x.double(), (256,), g_.double(), b_.double(), LN_EPS)
            en, en32 = (h.double() - n64).abs().max().item(), (F.layer_norm(x, (256,), g_, b_, LN_EPS).double() - n64).abs().max().item()
            if not within(en, en32, CHAIN_LN_FLOOR):
                failures.append(f"{fam}: the normalised rows {en:.3e} against max(4 x {en32:.3e}, {CHAIN_LN_FLOOR})")
        else:
            got, h = padded(lambda: ops.small_mlp(x, lay)), x
        e3, e32 = 0.0, 0.0
        for s_, (w, b, relu) in enumerate(lay):
            out = padded(lambda: ops.small_linear(h, w, b, relu=relu))

            def ref(dt):
                y = F.linear(h.to(dt), w.to(dt), b.to(dt) if b is not None else None)
                return y.relu() if relu else y
            scale = h.double().abs() @ w.double().abs().t() + (b.double().abs()[None] if b is not None else 0.0)
            ref64 = ref(torch.float64)
            es, es32 = rel_err(out, ref64, scale), rel_err(ref(torch.float32), ref64, scale)
            if not bound(es, es32):
                failures.append(f"{fam}: stage {s_} e3 {es:.3e} against max(4 x {es32:.3e}, 3e-7)")
            if es != es or (e3 == e3 and es >= e3):                                # the worst stage (a NaN stays)
                e3, e32 = es, es32
            h = out
        print("SR", name, fam, f"{e3:.3e} {e32:.3e}")
        if not torch.equal(got, h):
            failures.append(f"{fam}: not the bits of the chain of small_linear launches "
                            f"(largest difference {(got.double() - h.double()).abs().max().item():.3e})")
        if fam == "rows" and stages >= 2 and not in_ln:
            # the hidden row is zero: the output row is the last bias, bit for bit
            if not torch.equal(got[sr.CHAIN_DEAD_ROW], lay[-1][1]):
                failures.append(f"{fam}: the row behind a zero hidden row is not the last bias")
    assert not failures, name + ":\n  " + "\n  ".join(failures)


def test_small_mlp_bad_row_stays_in_its_row(cuda):
    M = 305
    x, lay = _chain_dev(M, 3, "rows", cuda)
    clean = padded(lambda: ops.small_mlp(x, lay))
    assert torch.isfinite(clean).all()
    for r in _bad_rows(M):
        assert r not in (sr.CHAIN_ZERO_ROW, sr.CHAIN_DEAD_ROW)
        for bad in (float("nan"), float("inf")):
            x2 = x.clone()
            x2[r, 133] = bad
            y = padded(lambda: ops.small_mlp(x2, lay))
            assert _others_equal(y, clean, r), (r, bad, "another row changed")
            assert torch.isnan(y[r]).all() if bad != bad else not torch.isfinite(y[r]).any(), (r, bad, y[r])


# ---- proca_attention ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.PROCA_CASES, ids=lambda v: "x".join(map(str, v)))
def test_proca_attention_family_against_fp64(cuda, case):
    Qp, L, T, h = case
    E = 32 * h
    failures = []
    for fam in sr.PROCA_FAMILIES:
        qkv0, kd, vd = (a.to(cuda) for a in sr.proca_inputs(case, fam))
        got = padded(lambda: ops.proca_attention(qkv0, kd, vd, h))
        assert tuple(got.shape) == (Qp * T, E)

        def ref(dt, want_scale=False):
            q, k0, v0 = qkv0.to(dt).view(Qp, T, 3, h, 32).unbind(2)                           # [Qp, T, h, d]
            k = torch.cat([k0[:, None], kd.to(dt).view(Qp, L, T, h, 32)], 1)                # [Qp, 1 + L, T, h, d]
            v = torch.cat([v0[:, None], vd.to(dt).view(Qp, L, T, h, 32)], 1)
            p = (torch.einsum("qthd,qlthd->qthl", q, k) / 32 ** 0.5).softmax(-1)
            out = torch.einsum("qthl,qlthd->qthd", p, v).reshape(Qp * T, E)
            return (out, torch.einsum("qthl,qlthd->qthd", p, v.abs()).reshape(Qp * T, E)) if want_scale else out
        ref64, scale = ref(torch.float64, True)
        e, e32 = rel_err(got, ref64, scale), rel_err(ref(torch.float32), ref64, scale)
        print("PA", "x".join(map(str, case)), fam, f"{e:.3e} {e32:.3e}")
        if not e < max(4.0 * e32, 2e-5):
            failures.append(f"{fam}: e {e:.3e} against max(4 x {e32:.3e}, 2e-5)")
        if fam == "uniform":
            v = torch.cat([qkv0[:, 2 * E:].view(Qp, 1, T, E), vd], 1).double()
            if not (ref64 - v.mean(1).reshape(Qp * T, E)).abs().max().item() < 1e-12:
                failures.append("uniform: the reference is not the mean of [v0; vd]")
    assert not failures, "\n  ".join(failures)
