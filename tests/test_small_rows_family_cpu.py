"""CPU: the tables of tests/small_rows_cases.py reach the paths of csrc/small_linear.hip they are named for, and the bound that
tests/test_small_rows_family_gpu.py asserts (e3 < max(4 e32, 3e-7), element-wise relative to |x + x_add| |W|^T + |b| + |residual|) is
one that the kernel's arithmetic itself keeps on exactly these inputs: a numpy restatement (the whole row's scale to 2^14, two fp16
parts per operand, three products per k-step, an fp32 accumulator rounded after each) stays at or below 1.5e-7, half the floor."""
import numpy as np
import pytest

from tests import small_rows_cases as sr


def test_case_ids_are_unique_and_every_case_has_a_path():
    assert len(sr.SL_BY_ID) == len(sr.SL_CASES) and set(sr.SL_PATHS) == set(sr.SL_BY_ID)
    assert set(sr.SL_BAD_ROW_CASES) <= set(sr.SL_BY_ID)


@pytest.mark.parametrize("c", sr.SL_CASES, ids=lambda c: c["id"])
def test_case_reaches_its_path_and_the_wrapper_covers_it(c):
    p = sr.launch(c)
    assert sr.SL_PATHS[c["id"]](p), (c["id"], p)
    # the checks of ops.small_linear and small_linear_f32 (csrc/small_linear.hip), restated: a listed case is never refused
    f_off, N = sr.feature_range(c)
    M, K, Nw = c["M"], c["K"], c["Nw"]
    assert 32 <= K <= 256 and K % 32 == 0 and N % 16 == 0 and Nw % 4 == 0 and f_off % 4 == 0 and 0 <= f_off and f_off + N <= Nw
    assert 1 <= M <= 4096 and M * K <= 4096 * 256 and M * N <= 4096 * 768
    assert c["add_features"] % 32 == 0 and (c["add_features"] == 0 or (c["x_add"] and c["add_features"] < N))
    assert not c["ln"] or N == 256
    assert c["out_T"] == 0 or (M % c["out_T"] == 0 and not c["residual"] and not c["ln"])


def test_the_table_holds_every_kind_of_workgroup_and_every_ragged_ring():
    tiles = [t for c in sr.SL_CASES for t in sr.launch(c)["tiles"]]
    assert sr.BOTH in tiles and sr.ADD_ONLY in tiles and sr.PLAIN_ONLY in tiles
    ks = {sr.launch(c)["KS"] for c in sr.SL_CASES}
    assert {1, 3, 5, 6, 7, 8} <= ks                       # every remainder of the SL_AHEAD = 4 ring, below and above one round
    assert {sr.launch(c)["KS"] % sr.SL_AHEAD for c in sr.SL_CASES} == {0, 1, 2, 3}
    assert any(sr.launch(c)["f_off_rem"] not in (0,) for c in sr.SL_CASES)
    assert any(sr.launch(c)["grid_y"] > 1 and 7 in sr.launch(c)["idle"].values() for c in sr.SL_CASES)


@pytest.mark.parametrize("c", [c for c in sr.SL_CASES if not c["ln"]], ids=lambda c: c["id"])
def test_numpy_restatement_keeps_half_the_floor(c):
    for fam in sr.families_of(c):
        t = sr.sl_inputs(c, fam)
        y, prod, ref, scale = sr.small_linear_np(c, t)
        assert np.isfinite(y).all()
        e3 = (np.abs(y.astype(np.float64) - ref) / (scale + 1e-300)).max()
        print("SRnp", c["id"], fam, f"{e3:.3e}")
        assert e3 <= 1.5e-7, (c["id"], fam, e3)
        if fam != "plain":
            assert (prod[3] == 0).all()                     # the zero row: exact


def test_a_neighbours_row_scale_breaks_the_bound():
    """The defect the element-wise measure is there for: a row scaled by the maximum of the next row of its 16-row tile.  The two fp16
    parts keep their 22 bits down to 2^-17 of the intended scale (fp16's exponent range), so a 30-fold neighbour
    (test_small_linear_matches_torch) costs nothing; on the `rows` family the rows 2^20 and more below their neighbour lose their
    second part -- far above the floor of the GPU file, and invisible relative to the largest output of the whole matrix."""
    c = sr.SL_BY_ID["ks7_n528"]
    M = c["M"]
    nb = np.minimum(np.arange(M) ^ 1, M - 1)
    t = sr.sl_inputs(c, "plain")
    t["x"][::3] *= 30.0
    t["xa"][::3] *= 30.0
    with np.errstate(all="ignore"):
        y, _, ref, scale = sr.small_linear_np(c, t, scale_from=nb)
    mx = np.abs(t["x"].numpy() + t["xa"].numpy()).max(1)
    small = mx * 8 < mx[nb]                                                          # (the other way round a row overflows fp16)
    assert small.sum() >= 4
    assert (np.abs(y.astype(np.float64) - ref) / scale)[small].max() <= 1.5e-7     # a 30-fold neighbour: nothing to see
    t = sr.sl_inputs(c, "rows")
    with np.errstate(all="ignore"):
        y, _, ref, scale = sr.small_linear_np(c, t, scale_from=nb)
    mx = np.abs(t["x"].numpy() + t["xa"].numpy()).max(1).astype(np.float64)
    small = (mx > 0) & (mx * 2.0 ** 20 <= mx[nb])                                    # scaled by a far larger neighbour: no overflow
    assert small.sum() >= 3 and np.isfinite(y[small]).all()
    err = np.abs(y.astype(np.float64) - ref)[small]
    assert (err / scale[small]).max() > 100 * 3e-7
    assert err.max() / max(1.0, np.abs(ref[np.isfinite(y).all(1)]).max()) < 2e-6


@pytest.mark.parametrize("c", [c for c in sr.SL_CASES if c["x_add"]], ids=lambda c: c["id"])
def test_cancel_rows_really_cancel(c):
    t = sr.sl_inputs(c, "cancel")
    idx = sr.cancel_rows(c["M"])
    assert idx and 3 not in idx
    x, xa = t["x"].numpy()[idx], t["xa"].numpy()[idx]
    s = (x + xa).astype(np.float32)
    assert (np.abs(s).max(1) / np.abs(x).max(1)).max() < 2.0 ** -9
    assert np.array_equal(s.astype(np.float64), x.astype(np.float64) + xa.astype(np.float64))      # the fp32 sum is exact
    # a 16-row tile of the `rows` family mixes many binades
    e = np.log2(np.abs(sr.sl_inputs(c, "rows")["x"].numpy()).max(1).astype(np.float64) + 1e-300)
    e = e[np.arange(c["M"]) != 3]
    assert e.max() - e.min() > 20 or c["M"] < 32


@pytest.mark.parametrize("M", sr.CHAIN_M)
@pytest.mark.parametrize("stages", (2, 3))
def test_chain_family_has_the_hidden_rows_it_names(M, stages):
    x, lay = sr.chain_inputs(M, stages, "rows")
    w1, b1, relu1 = lay[0]
    assert relu1 and (lay[1][1] is None) == (stages == 3)
    h = np.maximum(x.double().numpy() @ w1.double().numpy().T + b1.double().numpy()[None], 0.0)
    assert (h[sr.CHAIN_DEAD_ROW] == 0).all()                                          # the whole hidden row
    lo, hi = sr.CHAIN_DEAD_BLOCK
    dead = (h[:, lo:hi] == 0).all(1)
    alive = (h != 0).any(1)
    assert (dead & alive).sum() >= 2                                                  # rows with a whole zero k-step and other features
    even, odd = np.abs(h[:, 0::2]).max(1), np.abs(h[:, 1::2]).max(1)
    big = np.abs(x.numpy()).max(1) > 2.0 ** 5
    big[sr.CHAIN_DEAD_ROW] = False
    assert big.any() and (even[big] > 2.0 ** 20 * odd[big]).all()                    # 2^20 above the input; the odd features at b1's size


def test_proca_cases_sit_on_both_sides_of_the_lane_rounds():
    S = [1 + L for _, L, _, _ in sr.PROCA_CASES]
    assert {64, 65, 66, 128, 129} <= set(S) and {s % 2 for s in S} == {0, 1}
    assert max(S) * 4 == 64 * 1024                          # the largest L that proca_attention_f32 accepts
    for case in sr.PROCA_CASES[:2]:
        for fam in sr.PROCA_FAMILIES:
            qkv0, kd, vd = sr.proca_inputs(case, fam)
            Qp, L, T, h = case
            assert tuple(qkv0.shape) == (Qp * T, 96 * h) and tuple(kd.shape) == tuple(vd.shape) == (Qp, L, T, 32 * h)
            if fam == "offset":
                q = qkv0[:, :32 * h].reshape(Qp, T, h, 32).double()
                s = (q[:, None] * kd.reshape(Qp, L, T, h, 32).double()).sum(-1) / 32 ** 0.5
                assert 295 < s.min().item() and s.max().item() < 305
