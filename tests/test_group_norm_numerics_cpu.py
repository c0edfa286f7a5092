"""CPU: the statistics arithmetic of csrc/group_norm.hip restated in numpy fp32, run over the families and shapes of
tests/test_norm_conditioning_gpu.py with the same bound (err < max(4 * err32, 2e-5) against F.group_norm in fp64, err32 = ATen's fp32
result).  It is the error model behind that test and makes a change of the kernels' arithmetic change a test beside it.

What is restated (names as in group_norm.hip):
  gn_shift_sample /   the mean of 64 elements of the group, 8 consecutive ones from the middle of each of its 8 equal parts (index
  gn_shift            (2 (j / 8) + 1) n / 16 + j % 8, the last element where that is past the end), summed by the xor butterfly of
                      one wave;
  gn_partials_kernel  per plane and chunk (gn_chunks), 256 lanes sum d = x - shift and d * d in fp32 -- lane t takes float4 t,
                      t + 256, ... of the chunk on the vector path ((d.x + d.y) + (d.z + d.w), squares alike), element t, t + 256,
                      ... on the scalar path -- and block_sum_256 folds the lanes: the butterfly in each wave, then
                      lds[0] + lds[1] + lds[2] + lds[3];
  gn_apply_kernel /   lane i sums partials i, i + 256, ... of the group's Cg * chunks pairs, block_sum_256 again; m1 = s1 / n,
  gn_affine_kernel    var = max(s2 / n - m1 * m1, 0), mean = shift + m1, scale = gamma / sqrt(var + eps), bias = beta - mean * scale,
                      y = fma(x, scale, bias).
Not restated: which of the products the compiler fuses into FMAs (a fused product only drops a rounding)."""
import numpy as np
import pytest
import torch

from tests.test_norm_conditioning_gpu import FAMILIES, GN_CASES, GN_EPS, GN_FLOOR, gn_case, within

f32 = np.float32


def gn_chunks(C, groups, HW):
    Cg = C // groups
    chunks = max(1, (HW + 8191) // 8192)
    while chunks * Cg > 1024 and chunks > 1:
        chunks = (chunks + 1) // 2
    if chunks > 1:
        per = (HW + chunks - 1) // chunks
        if HW % 4 == 0 and per % 4 != 0:
            per4 = (per + 3) // 4 * 4
            chunks = (HW + per4 - 1) // per4
    return chunks


def butterfly64(v):
    """The xor butterfly of one wave over the last axis (64 lanes); every lane ends with the same value."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def block_sum_256(v):
    w = butterfly64(v.reshape(v.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def gn_shift(group):
    n = group.shape[-1]
    j = np.arange(64, dtype=np.int64)
    return butterfly64(group[..., np.minimum((2 * (j // 8) + 1) * n // 16 + j % 8, n - 1)]) * f32(1.0 / 64.0)


def first_element_shift(group):
    """What the kernels used before: a single element, so an outlier there brings the cancellation of E[x^2] - E[x]^2 back."""
    return group[..., 0]


def lane_sums(d, vec):
    """d [..., L] (a chunk, already shifted) -> the 256 lanes' (s1, s2) in the kernels' order."""
    L = d.shape[-1]
    step = 1024 if vec else 256
    K = (L + step - 1) // step
    d = np.concatenate([d, np.zeros(d.shape[:-1] + (K * step - L,), f32)], -1).reshape(d.shape[:-1] + ((K, 256, 4) if vec else (K, 256)))
    s1 = np.zeros(d.shape[:-1 - vec - 1] + (256,), f32)
    s2 = np.zeros_like(s1)
    for k in range(K):
        if vec:
            e = d[..., k, :, :]
            s1 = s1 + ((e[..., 0] + e[..., 1]) + (e[..., 2] + e[..., 3]))
            s2 = s2 + ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + (e[..., 2] * e[..., 2] + e[..., 3] * e[..., 3]))
        else:
            e = d[..., k, :]
            s1 = s1 + e
            s2 = s2 + e * e
    return s1, s2


def group_norm_restated(x, groups, gamma, beta, eps, shift_of=gn_shift):
    """x [N, C, H, W] float32 -> (y, scale [N, C], bias [N, C]) in the kernels' fp32 arithmetic."""
    N, C = x.shape[:2]
    HW = int(np.prod(x.shape[2:]))
    Cg = C // groups
    chunks = gn_chunks(C, groups, HW)
    per = (HW + chunks - 1) // chunks
    vec = HW % 4 == 0 and per % 4 == 0
    xg = x.reshape(N, groups, Cg, HW)
    shift = shift_of(xg.reshape(N, groups, Cg * HW)).astype(f32)                      # [N, groups]
    parts = []
    for c in range(chunks):
        d = xg[..., c * per:min((c + 1) * per, HW)] - shift[..., None, None]
        s1, s2 = lane_sums(d, vec)
        parts.append((block_sum_256(s1), block_sum_256(s2)))                          # [N, groups, Cg] each
    # the partials of a group in memory order: plane-major, chunk-minor
    p1 = np.stack([p[0] for p in parts], -1).reshape(N, groups, Cg * chunks)
    p2 = np.stack([p[1] for p in parts], -1).reshape(N, groups, Cg * chunks)
    K = (Cg * chunks + 255) // 256
    pad = np.zeros((N, groups, K * 256 - Cg * chunks), f32)
    l1 = np.concatenate([p1, pad], -1).reshape(N, groups, K, 256)
    l2 = np.concatenate([p2, pad], -1).reshape(N, groups, K, 256)
    s1, s2 = np.zeros((N, groups, 256), f32), np.zeros((N, groups, 256), f32)
    for k in range(K):
        s1, s2 = s1 + l1[:, :, k], s2 + l2[:, :, k]
    s1, s2 = block_sum_256(s1), block_sum_256(s2)
    inv_n = f32(1.0) / (f32(Cg) * f32(HW))
    m1 = s1 * inv_n
    var = np.maximum(s2 * inv_n - m1 * m1, f32(0.0))
    mean = shift + m1
    rstd_den = np.sqrt(var + f32(eps))                                                # [N, groups]
    scale = gamma.reshape(1, groups, Cg) / rstd_den[..., None]
    bias = beta.reshape(1, groups, Cg) - mean[..., None] * scale
    assert scale.dtype == f32 and bias.dtype == f32
    y = (xg.astype(np.float64) * scale[..., None].astype(np.float64) + bias[..., None].astype(np.float64)).astype(f32)   # one rounding: fma
    return y.reshape(x.shape), scale.reshape(N, C), bias.reshape(N, C)


def restated_error(case, fam, shift_of=gn_shift):
    shape, groups = case
    x, w, b, ref, err32 = gn_case(shape, groups, fam)
    y, _, _ = group_norm_restated(x.numpy(), groups, w.numpy(), b.numpy(), GN_EPS, shift_of)
    assert np.isfinite(y).all()
    return np.abs(y.astype(np.float64) - ref.numpy()).max(), err32, y


def test_gn_chunks_reaches_every_path():
    """The shapes of the conditioning tests are what their comments say: one and two chunks, both load paths, the re-chunking branch."""
    chunks = [gn_chunks(s[1], g, s[2] * s[3]) for s, g in GN_CASES]
    assert chunks == [1, 1, 2, 2, 2, 1]
    vec = [(s[2] * s[3]) % 4 == 0 and ((s[2] * s[3] + c - 1) // c) % 4 == 0 for (s, g), c in zip(GN_CASES, chunks)]
    assert vec == [True, False, True, False, False, False]
    HW = 12 * 683                       # the plane is 16-B aligned, its halves are not: gn_chunks' re-chunking branch runs
    assert HW % 4 == 0 and ((HW + 1) // 2) % 4 != 0


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("case", GN_CASES, ids=lambda v: "x".join(map(str, v[0])) + f"g{v[1]}")
def test_restated_group_norm_holds_the_bound(case, fam):
    err, err32, y = restated_error(case, fam)
    print(f"restated group_norm {case} {fam}: {err:.2e} (ATen fp32 {err32:.2e})")
    assert within(err, err32, GN_FLOOR), (err, err32)
    if fam == "constant":
        _, w, b, _, _ = gn_case(case[0], case[1], fam)
        tol = np.spacing(f32(3.25) * w.abs().max().numpy() / np.sqrt(f32(GN_EPS)))
        assert np.abs(y - b.numpy().reshape(1, -1, 1, 1)).max() <= tol


@pytest.mark.parametrize("case", GN_CASES, ids=lambda v: "x".join(map(str, v[0])) + f"g{v[1]}")
def test_restated_outlier_position_does_not_matter(case):
    e_first, e_last = restated_error(case, "first_outlier100")[0], restated_error(case, "last_outlier100")[0]
    assert max(e_first, e_last) < GN_FLOOR or max(e_first, e_last) <= 4.0 * min(e_first, e_last), (e_first, e_last)


def test_single_element_shift_does_not_hold_the_bound():
    """Why the shift is a sample mean: with the group's first element as the shift the same arithmetic loses two and more digits as
    soon as that element is an outlier, while an outlier elsewhere costs nothing."""
    case = GN_CASES[2]
    for fam in ("first_outlier30", "first_outlier100", "offset_first_zero"):
        err, err32, _ = restated_error(case, fam, first_element_shift)
        assert err > 10.0 * max(4.0 * err32, GN_FLOOR), (fam, err, err32)
    err, err32, _ = restated_error(case, "last_outlier100", first_element_shift)
    assert within(err, err32, GN_FLOOR)
