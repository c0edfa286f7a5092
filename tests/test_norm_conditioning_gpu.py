"""GPU: the normalisation kernels (csrc/group_norm.hip, layer_norm.hip, the LayerNorm epilogues of transpose.hip, small_linear.hip and
mlp_f16x3.hip, softmax.hip) on ill-conditioned groups and rows: mean >> std, one outlier at the first / last element, zero variance,
scales far from 1.  The reference is the same operation in fp64 on the CPU; the bound is the project's usual one,
err < max(4 * err32, floor), err32 being ATen's fp32 result against the same fp64 reference on the same input and floor the figure of
the neighbouring test in tests/test_ops_gpu.py.  No per-family tolerance: ATen's own error grows with the family (about 1e-4 at
`big_mean`) and the bound follows it.  tests/test_group_norm_numerics_cpu.py checks the same families and shapes on a numpy
restatement of group_norm.hip's arithmetic."""
import functools

import numpy as np
import pytest
import torch

from univs_amd import ops, synth

pytestmark = pytest.mark.gpu

F = torch.nn.functional

FAMILIES = ("benign", "first_outlier10", "first_outlier30", "first_outlier100", "last_outlier100", "offset_first_zero", "big_mean",
            "constant", "tiny", "huge", "sparse")


def family(name, tag, units, length):
    """[units, length] float32, one line per GroupNorm group or LayerNorm row; every family is a function of the same
    synth.normal base `z` of (tag, units, length).
      benign             z * 2 + 0.7 (what the neighbouring tests feed: the anchor)
      first_outlier<k>   benign with the first element of every line at mean + k std = 0.7 + 2 k
      last_outlier<k>    the same value on the last element (the control: the position of an element must not matter)
      offset_first_zero  N(50, 1) with the first element 0, as a zero-padded image corner
      big_mean           N(1000, 1)
      constant           3.25 everywhere: variance 0
      tiny               N(5, (1e-3)^2): eps matters
      huge               N(0, (1e4)^2)
      sparse             relu(z - 2.5) * 5 with the first element 40"""
    z = synth.normal(f"cond/{tag}/{units}x{length}", (units, length))
    if name == "benign":
        return z * 2.0 + 0.7
    if name.startswith("first_outlier") or name.startswith("last_outlier"):
        x = z * 2.0 + 0.7
        x[:, 0 if name.startswith("first") else -1] = 0.7 + 2.0 * float(name.split("outlier")[1])
        return x
    if name == "offset_first_zero":
        x = z + 50.0
        x[:, 0] = 0.0
        return x
    if name == "big_mean":
        return z + 1000.0
    if name == "constant":
        return torch.full_like(z, 3.25)
    if name == "tiny":
        return z * 1e-3 + 5.0
    if name == "huge":
        return z * 1e4
    if name == "sparse":
        x = torch.relu(z - 2.5) * 5.0
        x[:, 0] = 40.0
        return x
    raise KeyError(name)


def max_err(got, ref64):
    return (got.detach().cpu().double() - ref64.cpu()).abs().max().item()


def within(err, err32, floor=2e-5):
    return err < max(4.0 * err32, floor)


# ---- GroupNorm ---------------------------------------------------------------------------------------------------------------------------
# the smallest shapes that reach each path of gn_chunks and both load paths of the kernels
GN_CASES = [((2, 32, 23, 40), 4),      # one chunk, vector path
            ((3, 32, 7, 9), 8),        # one chunk, scalar path
            ((1, 16, 92, 92), 2),      # HW = 8464: 2 chunks of 4232, vector path
            ((1, 8, 12, 683), 4),      # HW = 8196, HW % 4 == 0 but per = 4098 is not: the re-chunking branch (2 chunks again: scalar path)
            ((1, 8, 91, 93), 4),       # HW = 8463: 2 chunks, scalar path
            ((2, 16, 1, 1), 4)]        # a group of 4 values
GN_EPS = 1e-5
GN_FLOOR = 2e-5                        # test_group_norm_matches_torch


@functools.lru_cache(maxsize=None)
def gn_case(shape, groups, fam):
    """(x, weight, bias, fp64 reference, err32) of one GroupNorm case on the CPU; computed once, shared, never written to."""
    N, C = shape[:2]
    hw = int(np.prod(shape[2:]))
    x = family(fam, "gn", N * groups, (C // groups) * hw).reshape(shape).contiguous()
    w = 1.0 + 0.1 * synth.uniform(f"gn/w/{C}", (C,))
    b = 0.05 * synth.uniform(f"gn/b/{C}", (C,))
    ref = F.group_norm(x.double(), groups, w.double(), b.double(), GN_EPS)
    err32 = max_err(F.group_norm(x, groups, w, b, GN_EPS), ref)
    return x, w, b, ref, err32


def _gn_id(v):
    return "x".join(map(str, v[0])) + f"g{v[1]}"


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("case", GN_CASES, ids=_gn_id)
def test_group_norm_conditioning(cuda, case, fam):
    """ops.group_norm (with and without ReLU), the (scale, bias) pairs of ops.group_norm_affine and the two consumers that apply them
    while they read x (upsample2x_add, tokens_from_nchw) against F.group_norm in fp64."""
    shape, groups = case
    x, w, b, ref, err32 = gn_case(shape, groups, fam)
    N, C, H, W = shape
    xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
    y = ops.group_norm(xd, groups, wd, bd, GN_EPS)
    yr = ops.group_norm(xd, groups, wd, bd, GN_EPS, relu=True)
    aff = ops.group_norm_affine(xd, groups, wd, bd, GN_EPS)
    assert tuple(aff.shape) == (N * C, 2)
    a64 = aff.cpu().double().view(N, C, 2, 1, 1)
    e_y, e_r = max_err(y, ref), max_err(yr, torch.relu(ref))
    e_a = (x.double() * a64[:, :, 0] + a64[:, :, 1] - ref).abs().max().item()
    print(f"group_norm {shape} g={groups} {fam}: {e_y:.2e} relu {e_r:.2e} affine {e_a:.2e} (ATen fp32 {err32:.2e})")
    assert torch.isfinite(y).all() and torch.isfinite(aff).all()
    assert within(e_y, err32, GN_FLOOR), (e_y, err32)
    assert within(e_r, err32, GN_FLOOR), (e_r, err32)
    assert within(e_a, err32, GN_FLOOR), (e_a, err32)
    if fam == "constant":
        # every element equals the mean: the output is beta up to the one rounding the affine form y = x * scale + bias has, that of
        # bias = beta - mean * scale at the magnitude of mean * scale = 3.25 gamma / sqrt(eps) (the fused consumers take that form)
        tol = np.spacing(np.float32(3.25) * w.abs().max().numpy() / np.sqrt(np.float32(GN_EPS)))
        assert (y.cpu() - b.view(1, C, 1, 1)).abs().max().item() <= float(tol)
    if H % 2 == 0 and W % 4 == 0:
        # the FPN top-down step with the ill-conditioned map as the addend: bit-identical to the two launches it replaces
        xs = synth.normal("cond/up/" + "x".join(map(str, shape)), (N, C, H // 2, W // 2)).to(cuda)
        fused = ops.upsample2x_add(xs, xd, aff)
        assert fused is not None and torch.equal(fused, ops.bilinear_resample(xs, (H, W), addend=y))
    if (H * W) % 4 == 0 and C % 4 == 0:
        tok = ops.tokens_from_nchw([xd], [aff], None)
        assert tok is not None and tok[1] is None
        e_t = max_err(tok[0], ref.flatten(2).transpose(1, 2))
        e_ty = (tok[0] - y.flatten(2).transpose(1, 2)).abs().max().item()
        print(f"  tokens_from_nchw: {e_t:.2e} vs fp64, {e_ty:.2e} vs group_norm")
        assert within(e_t, err32, GN_FLOOR) and within(e_ty, err32, GN_FLOOR), (e_t, e_ty, err32)


@pytest.mark.parametrize("case", GN_CASES, ids=_gn_id)
def test_group_norm_outlier_position_does_not_matter(cuda, case):
    """The same outlier at the first and at the last element of every group: errors within a factor 4 of each other, or both below
    the floor."""
    shape, groups = case
    errs = []
    for fam in ("first_outlier100", "last_outlier100"):
        x, w, b, ref, _ = gn_case(shape, groups, fam)
        errs.append(max_err(ops.group_norm(x.to(cuda), groups, w.to(cuda), b.to(cuda), GN_EPS), ref))
    print(f"group_norm {shape} g={groups}: first {errs[0]:.2e} last {errs[1]:.2e}")
    assert max(errs) < GN_FLOOR or max(errs) <= 4.0 * min(errs), errs


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
LN_EPS = 1e-5
LN_FLOOR = 2e-5                        # test_layer_norm_matches_torch


def _ln_params(C, tag="ln"):
    return 1.0 + 0.1 * synth.uniform(f"cond/{tag}/w/{C}", (C,)), 0.05 * synth.uniform(f"cond/{tag}/b/{C}", (C,))


def _ln_check(what, got, rows64, w, b, floor=LN_FLOOR):
    """`got` against F.layer_norm of the fp64 rows; err32 = ATen's fp32 LayerNorm of the same rows (given in fp32)."""
    C = rows64.shape[-1]
    ref = F.layer_norm(rows64.cpu(), (C,), w.cpu().double(), b.cpu().double(), LN_EPS)
    err32 = max_err(F.layer_norm(rows64.cpu().float(), (C,), w.cpu(), b.cpu(), LN_EPS), ref)
    err = max_err(got, ref)
    print(f"{what}: {err:.2e} (ATen fp32 {err32:.2e})")
    assert torch.isfinite(got).all()
    assert within(err, err32, floor), (what, err, err32)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("C", [96, 256, 768, 3072])
@pytest.mark.parametrize("rows", [7, 65])
def test_layer_norm_conditioning(cuda, rows, C, fam):
    """ops.layer_norm on every (G, NV) class of layer_norm.hip: plain, with the fused residual and the returned sum (the reference
    normalises the fp32 sum in fp64), and the second-output form.  (`constant` at C = 96 is what made the kernels divide by C: with
    mean = sum * (1 / C) the mean of 96 equal values was one ulp off, every deviation non-zero and the output 3.4e-5 from beta, where
    ATen gives beta exactly.)"""
    x = family(fam, "ln", rows, C)
    r = synth.normal(f"cond/ln/r/{rows}/{C}", (rows, C))
    p = synth.normal(f"cond/ln/p/{rows}/{C}", (rows, C))
    w, b = _ln_params(C)
    xd, rd, pd, wd, bd = (t.to(cuda) for t in (x, r, p, w, b))
    _ln_check(f"layer_norm {rows}x{C} {fam}", ops.layer_norm(xd, wd, bd, LN_EPS), x.double(), w, b)
    s, y = ops.layer_norm(xd, wd, bd, LN_EPS, residual=rd, return_sum=True)
    assert torch.equal(s.cpu(), x + r)
    _ln_check(f"layer_norm {rows}x{C} {fam} + residual", y, (x + r).double(), w, b)
    out, out2 = ops.layer_norm(xd, wd, bd, LN_EPS, residual=rd, post_add=pd)
    assert torch.equal(out, y) and torch.equal(out2, y + pd)


@pytest.mark.parametrize("C", [96, 256, 768, 3072])
@pytest.mark.parametrize("rows", [7, 65])
def test_layer_norm_residual_cancels(cuda, rows, C):
    """x = big, r = -big + normal: the sum is the fp32 sum bit for bit, and its LayerNorm is that of the small remainder."""
    big = (synth.normal(f"cond/ln/big/{rows}/{C}", (rows, C)).abs() + 1.0) * 1e4
    r = -big + synth.normal(f"cond/ln/rem/{rows}/{C}", (rows, C))
    w, b = _ln_params(C)
    s, y = ops.layer_norm(big.to(cuda), w.to(cuda), b.to(cuda), LN_EPS, residual=r.to(cuda), return_sum=True)
    assert torch.equal(s.cpu(), big + r)
    _ln_check(f"layer_norm {rows}x{C} big - big", y, (big + r).double(), w, b)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("shape", [(1, 6, 10, 96), (2, 5, 7, 192)], ids=lambda v: "x".join(map(str, v)))
def test_patch_merge_norm_conditioning(cuda, shape, fam):
    """ops.patch_merge_norm with the family on the merged 4 C rows (the zero padding of odd sizes stays zero)."""
    B, H, W, C = shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    m = family(fam, "pm", B * H2 * W2, 4 * C).view(B, H2, W2, 4, C)
    xp = torch.zeros(B, 2 * H2, 2 * W2, C)
    xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2] = m[..., 0, :], m[..., 1, :], m[..., 2, :], m[..., 3, :]
    x = xp[:, :H, :W].contiguous()
    xp = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    cat = torch.cat([xp[:, 0::2, 0::2, :], xp[:, 1::2, 0::2, :], xp[:, 0::2, 1::2, :], xp[:, 1::2, 1::2, :]], -1).reshape(B, -1, 4 * C)
    w, b = _ln_params(4 * C, "pm")
    y = ops.patch_merge_norm(x.to(cuda), w.to(cuda), b.to(cuda), LN_EPS)
    assert y is not None and tuple(y.shape) == tuple(cat.shape)
    _ln_check(f"patch_merge_norm {shape} {fam}", y, cat.double(), w, b)
    assert torch.equal(y, ops.layer_norm(cat.to(cuda), w.to(cuda), b.to(cuda), LN_EPS))


@pytest.mark.parametrize("fam", ["benign", "big_mean", "first_outlier30", "first_outlier100"])
def test_patch_embed4_norm_conditioning(cuda, fam):
    """The LayerNorm of ops.patch_embed4 at (2, 16, 24, 96) with embedded rows that follow the family: the taps of every filter sum
    to 1, so pixels ~ N(1000, 1) give rows of mean 1000 and O(1) spread; the outlier sits in the first channel (its bias).
    Reference: convolution and LayerNorm in fp64; err32: ATen's fp32 convolution and LayerNorm."""
    T, H, W, E = 2, 16, 24, 96
    x = synth.normal("cond/pe4/x", (T, 3, H, W)) * 2.0
    w = synth.normal("cond/pe4/w", (E, 3, 4, 4), std=48 ** -0.5)
    b = synth.normal("cond/pe4/b", (E,), std=0.3)
    if fam == "big_mean":
        x = x * 0.5 + 1000.0
        w = w - w.mean(dim=(1, 2, 3), keepdim=True) + 1.0 / 48.0
    elif fam.startswith("first_outlier"):
        b[0] = 2.0 * float(fam.split("outlier")[1])
    g_, be = _ln_params(E, "pe4")
    got = ops.patch_embed4(x.to(cuda), w.to(cuda), b.to(cuda), (g_.to(cuda), be.to(cuda), LN_EPS))
    assert got is not None and tuple(got.shape) == (T, (H // 4) * (W // 4), E)
    rows64 = F.conv2d(x.double(), w.double(), b.double(), stride=4).flatten(2).transpose(1, 2)
    ref = F.layer_norm(rows64, (E,), g_.double(), be.double(), LN_EPS)
    ref32 = F.layer_norm(F.conv2d(x, w, b, stride=4).flatten(2).transpose(1, 2), (E,), g_, be, LN_EPS)
    err, err32 = max_err(got, ref), max_err(ref32, ref)
    print(f"patch_embed4 + LN {fam}: rows mean {rows64.mean().item():.1f} std {rows64.std(-1).mean().item():.2f}: {err:.2e} "
          f"(ATen fp32 {err32:.2e})")
    assert within(err, err32, 2e-5), (err, err32)          # floor: test_patch_embed4_matches_torch


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("M,K,add,relu", [(500, 256, False, False), (300, 128, True, True)], ids=lambda v: str(v))
def test_small_linear_norm_conditioning(cuda, M, K, add, relu, fam):
    """The `ln=` epilogue of ops.small_linear (norm(tgt + out_proj(.)), shapes of test_small_linear_matches_torch) with the family on
    the residual rows and an O(1) product; reference and err32 are the fp64 / ATen fp32 compositions of the same ops, the error
    relative to max(1, |ref|) and the floor 2e-6 as there."""
    N = 256
    tag = f"cond/sl/{M}x{K}"
    x, xa = synth.normal(tag + "/x", (M, K)), synth.normal(tag + "/xa", (M, K))
    w, b = synth.normal(tag + "/w", (N, K), std=K ** -0.5), synth.normal(tag + "/b", (N,), std=0.5)
    r = family(fam, "sl", M, N)
    g_, be = 1.0 + 0.2 * synth.normal(tag + "/g", (N,)), 0.1 * synth.normal(tag + "/be", (N,))
    xd, xad, wd, bd, rd, gd, bed = (t.to(cuda) for t in (x, xa, w, b, r, g_, be))
    y = ops.small_linear(xd, wd, bd, x_add=xad if add else None, relu=relu, residual=rd, ln=(gd, bed, LN_EPS))
    assert y is not None and tuple(y.shape) == (M, N)

    def ref(dt):
        c = lambda t: t.to(dt)
        t = F.linear(c(xd) + c(xad) if add else c(xd), c(wd), c(bd))
        return F.layer_norm((F.relu(t) if relu else t) + c(rd), (N,), c(gd), c(bed), LN_EPS)
    ref64, ref32 = ref(torch.float64), ref(torch.float32)
    scale = max(1.0, ref64.abs().max().item())
    err, err32 = max_err(y, ref64) / scale, max_err(ref32, ref64) / scale
    print(f"small_linear + LN {M, K} {fam}: {err:.2e} (ATen fp32 {err32:.2e}), scale {scale:.1f}")
    assert torch.isfinite(y).all() and within(err, err32, 2e-6), (err, err32)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("N,S,C,Hd", [(3, 1111, 256, 512), (1, 4000, 192, 384)], ids=lambda v: str(v))
def test_mlp_fused_post_norm_conditioning(cuda, N, S, C, Hd, fam):
    """The post-norm of the fused MLP, LayerNorm(residual + linear2(relu(linear1(x)))) (shapes of test_mlp_fused_post_norm), with the
    family on the residual rows and an O(1) product; the fp64 / ATen fp32 compositions and the floor 5e-6 as there."""
    tag = f"cond/mlp/{N}x{S}x{C}"
    x = synth.normal(tag + "/x", (N, S, C))
    r = family(fam, "mlp", N * S, C).view(N, S, C)
    g_, b_ = 1.0 + 0.2 * synth.normal(tag + "/g", (C,)), 0.1 * synth.normal(tag + "/b", (C,))
    w1, b1 = synth.normal(tag + "/w1", (Hd, C), std=C ** -0.5), synth.normal(tag + "/b1", (Hd,), std=0.5)
    w2, b2 = synth.normal(tag + "/w2", (C, Hd), std=Hd ** -0.5), synth.normal(tag + "/b2", (C,), std=0.5)
    xd, rd, gd, bd, w1d, b1d, w2d, b2d = (t.to(cuda) for t in (x, r, g_, b_, w1, b1, w2, b2))
    y = ops.mlp_fused(xd, w1d, b1d, w2d, b2d, "relu", residual=rd, post_ln=(gd, bd, LN_EPS))
    assert y is not None and tuple(y.shape) == (N, S, C)

    def ref(dt):
        c = lambda t: t.to(dt)
        return F.layer_norm(c(rd) + F.linear(F.relu(F.linear(c(xd), c(w1d), c(b1d))), c(w2d), c(b2d)), (C,), c(gd), c(bd), LN_EPS)
    ref64 = ref(torch.float64)
    err, err32 = max_err(y, ref64), max_err(ref(torch.float32), ref64)
    print(f"mlp_fused post-norm {N, S, C, Hd} {fam}: {err:.2e} (ATen fp32 {err32:.2e})")
    assert torch.isfinite(y).all() and within(err, err32, 5e-6), (err, err32)


# ---- masked softmax ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["offset_1e4", "spread_60"])
@pytest.mark.parametrize("N,h,L,S", [(3, 4, 7, 33), (1, 2, 5, 14720)], ids=lambda v: str(v))
def test_masked_softmax_conditioning(cuda, N, h, L, S, kind):
    """ops.masked_softmax_ against the fp64 softmax at the 4e-6 of test_masked_softmax_matches_torch: scores of that test shifted by
    1e4, scores spread over +-60 (exp underflows), and in both a row whose single unmasked key holds the row's minimum."""
    x = synth.normal(f"sm/x/{N}/{h}/{L}/{S}", (N, h, L, S)) * 3.0 + 1e4 if kind == "offset_1e4" else \
        synth.uniform(f"cond/sm/x/{N}/{h}/{L}/{S}", (N, h, L, S)) * 60.0
    m = synth.uniform(f"sm/m/{N}/{L}/{S}", (N, L, S)) > 0.3
    m[..., 0] = False                       # no fully masked row
    m[:, 0, :] = True                       # row 0 of every image: one key left, below every masked one
    m[:, 0, S // 2] = False
    x[:, :, 0, S // 2] = x.min() - 1.0
    ref = torch.softmax(x.double().masked_fill(m.unsqueeze(1), float("-inf")), dim=-1)
    assert torch.equal(ref[:, :, 0, S // 2], torch.ones(N, h, dtype=torch.float64))
    got = ops.masked_softmax_(x.to(cuda), m.to(cuda)).cpu()
    err = max_err(got, ref)
    got2 = ops.masked_softmax_(x.to(cuda), None).cpu()
    err2 = max_err(got2, torch.softmax(x.double(), dim=-1))
    print(f"masked_softmax {N, h, L, S} {kind}: masked {err:.2e} unmasked {err2:.2e}")
    assert torch.isfinite(got).all() and err < 4e-6 and err2 < 4e-6, (err, err2)
