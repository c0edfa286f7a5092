"""The few-rows kernels of the decoder (csrc/small_linear.hip: small_linear_kernel<false>, small_chain_kernel; csrc/proca_attn.hip) at
their tile edges and over wide row ranges: the case tables, the input families and the launch arithmetic of a case restated from
the kernel.  A plain module like tests/gemm_instances.py, read by tests/test_small_rows_family_cpu.py (every case reaches the path it
is named for; the bound of the GPU file holds for a numpy restatement of the kernel's arithmetic on exactly these inputs) and
tests/test_small_rows_family_gpu.py (every case and family against fp64).

A small_linear case is (M, K, Nw, rows = (f_off, N) | None, x_add, add_features, relu, residual, ln, out_T): the smallest shape that
reaches its path.  How to add one: append it to SL_CASES with the predicate its path needs in SL_PATHS, run the CPU file, then the
GPU file."""
import zlib

SL_WG_FEATURES = 256       # 8 waves x 32 features (small_linear.hip: SL_WAVES)
SL_AHEAD = 4               # k-steps of weight fragments in flight


def _sl(id_, M, K, Nw, rows, x_add, add_features, relu, residual, ln, out_T):
    return {"id": id_, "M": M, "K": K, "Nw": Nw, "rows": rows, "x_add": bool(x_add), "add_features": add_features, "relu": bool(relu),
            "residual": bool(residual), "ln": bool(ln), "out_T": out_T}


SL_CASES = [
    _sl("ks1_n16", 33, 32, 16, None, 0, 0, 0, 0, 0, 0),
    _sl("ks3_n48", 17, 96, 48, None, 1, 0, 1, 0, 0, 0),
    _sl("ks5_n272", 100, 160, 272, None, 0, 0, 0, 1, 0, 0),
    _sl("ks7_n528", 47, 224, 528, None, 1, 0, 1, 1, 0, 0),
    _sl("straddle32", 64, 192, 320, (20, 288), 1, 32, 0, 0, 0, 0),
    _sl("straddle288", 250, 256, 640, (4, 576), 1, 288, 0, 1, 0, 0),
    _sl("ln_rows", 305, 256, 256, None, 1, 0, 0, 1, 1, 0),
    _sl("transposed", 35, 64, 48, None, 1, 0, 1, 0, 0, 7),
    _sl("decoder_qkv", 500, 256, 768, (0, 768), 1, 512, 0, 0, 0, 0),
]
SL_BY_ID = {c["id"]: c for c in SL_CASES}
SL_FAMILIES = ("plain", "rows", "cancel")
SL_BAD_ROW_CASES = ("ks7_n528", "straddle288", "ln_rows")

CHAIN_M = (17, 305)
CHAIN_STAGES = (1, 2, 3)
CHAIN_FAMILIES = ("plain", "rows")
CHAIN_ZERO_ROW, CHAIN_DEAD_ROW = 3, 5       # x[3] = 0; x[5] drives every hidden feature below zero (two stages and more)
CHAIN_DEAD_BLOCK = (64, 96)                 # features of b1 that are far below zero: k-step 2 of the second stage

PROCA_CASES = [(2, 63, 3, 8), (2, 64, 1, 8), (1, 65, 2, 2), (3, 127, 2, 1), (1, 128, 5, 8), (1, 16383, 1, 1)]
PROCA_FAMILIES = ("plain", "sharp", "uniform", "own_state", "last_key", "offset", "v_range_1e6", "v_range_1e-6", "v_range_tokens")


def families_of(c):
    return tuple(f for f in SL_FAMILIES if f != "cancel" or c["x_add"])


def feature_range(c):
    return (0, c["Nw"]) if c["rows"] is None else c["rows"]


# ---- the launch arithmetic of small_linear_f32 / small_linear_kernel<false>, restated
def launch(c):
    """KS, grid.y, per workgroup column (need_add, need_plain), per (column, wave) with features its f_ok1, M % 16, f_off % 16"""
    f_off, N = feature_range(c)
    af, add = c["add_features"], c["x_add"]
    grid_y = (N + SL_WG_FEATURES - 1) // SL_WG_FEATURES
    tiles, f_ok1, idle = [], {}, {}
    for by in range(grid_y):
        fbase = by * SL_WG_FEATURES
        fend = min(fbase + SL_WG_FEATURES, N)
        tiles.append((add and (af == 0 or fbase < af), (not add) or (af != 0 and fend > af)))
        idle[by] = 0
        for wave in range(8):
            f0 = fbase + 32 * wave
            if f0 >= N:
                idle[by] += 1                    # (`if (f0 >= N && !with_ln) return;`)
            else:
                f_ok1[(by, wave)] = f0 + 16 < N
    # the operand tile a wave reads: 0 = x + x_add, 1 = x
    my_tile = {bw: 0 if (add and (af == 0 or bw[0] * SL_WG_FEATURES + 32 * bw[1] < af)) else 1 for bw in f_ok1}
    return {"KS": c["K"] // 32, "grid_y": grid_y, "tiles": tiles, "f_ok1": f_ok1, "idle": idle, "my_tile": my_tile, "m_rem": c["M"] % 16,
            "f_off_rem": f_off % 16, "ragged_ring": (c["K"] // 32) % SL_AHEAD != 0}


BOTH, ADD_ONLY, PLAIN_ONLY = (True, True), (True, False), (False, True)

# the path table: what the case named for a row has to reach
SL_PATHS = {
    "ks1_n16": lambda p: p["KS"] == 1 < SL_AHEAD and p["grid_y"] == 1 and list(p["f_ok1"]) == [(0, 0)] and not p["f_ok1"][(0, 0)]
    and p["idle"][0] == 7 and p["m_rem"] == 1,
    "ks3_n48": lambda p: p["KS"] == 3 and p["ragged_ring"] and p["f_ok1"][(0, 0)] and not p["f_ok1"][(0, 1)] and p["tiles"] == [ADD_ONLY],
    "ks5_n272": lambda p: p["KS"] == 5 and p["ragged_ring"] and p["grid_y"] == 2 and p["idle"][1] == 7 and not p["f_ok1"][(1, 0)],
    "ks7_n528": lambda p: p["KS"] == 7 and p["ragged_ring"] and p["grid_y"] == 3 and p["idle"][2] == 7 and not p["f_ok1"][(2, 0)],
    "straddle32": lambda p: p["KS"] == 6 and p["ragged_ring"] and p["f_off_rem"] == 4 and p["tiles"] == [BOTH, PLAIN_ONLY]
    and [p["my_tile"][(0, w)] for w in range(8)] == [0] + [1] * 7,
    "straddle288": lambda p: p["tiles"] == [ADD_ONLY, BOTH, PLAIN_ONLY] and p["f_off_rem"] == 4
    and [p["my_tile"][(1, w)] for w in range(8)] == [0] + [1] * 7,
    "ln_rows": lambda p: p["m_rem"] == 1 and p["grid_y"] == 1 and p["idle"][0] == 0,
    "transposed": lambda p: p["m_rem"] == 3 and p["KS"] == 2,
    "decoder_qkv": lambda p: p["tiles"] == [ADD_ONLY, ADD_ONLY, PLAIN_ONLY] and p["KS"] == 8 and not p["ragged_ring"],
}


# ---- inputs (torch's CPU generator, seeded from the case's id as gemm_instances.plain_inputs does)
def _gen(tag):
    import torch
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def _row_powers(tag, M):
    import torch
    return torch.exp2(torch.randint(-30, 31, (M, 1), generator=_gen("rows/" + tag)).float())       # exact powers of two


def cancel_rows(M):
    return list(range(7, M, 5))


def sl_inputs(c, family):
    """{x, xa, w, b, r, g, be} on the CPU.
      plain   gemm_instances.plain_inputs (x ~ N(0, 1), w ~ N(0, 1 / K), b ~ N(0, 1 / 4), r ~ N(0, 1)), x_add ~ N(0, 1)
      rows    plain with x, x_add and the residual times the same power of two per row from 2^-30 .. 2^30 (a 16-row tile mixes magnitudes
              over many binades), the rows of W times logspace(-3, 3, Nw); row 3 is zero in x and x_add
      cancel  rows, but every 5th row from row 7 has x_add = -x (1 + 2^-12 z): the operand is ~2^-12 of either summand"""
    import torch
    from tests.gemm_instances import plain_inputs
    M, K, Nw = c["M"], c["K"], c["Nw"]
    _, N = feature_range(c)
    x, w, b, _ = plain_inputs(M, K, Nw, "sr/" + c["id"])
    g = _gen(f"sr/{c['id']}/more")
    xa, r = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    gam, bet = 1.0 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    if family != "plain":
        assert family in ("rows", "cancel"), family
        p = _row_powers(c["id"], M)
        x, xa, r = x * p, xa * p, r * p
        w = w * torch.logspace(-3, 3, Nw).view(Nw, 1)
        x[3], xa[3] = 0.0, 0.0
        if family == "cancel":
            z = torch.randn(M, K, generator=g)
            idx = cancel_rows(M)
            xa[idx] = -(x[idx] * (1.0 + 2.0 ** -12 * z[idx]))
    return {"x": x, "xa": xa if c["x_add"] else None, "w": w, "b": b, "r": r if c["residual"] else None, "g": gam, "be": bet}


def chain_inputs(M, stages, family):
    """(x [M, 256], [(W, b | None, relu)] * stages) on the CPU; ReLU between the stages, the middle Linear of three without a bias (as
    the MLP test of tests/test_ops_gpu.py).
      plain   x ~ N(0, 1), W ~ N(0, 1 / 256), b ~ N(0, 1 / 4)
      rows    x times a power of two per row from 2^-30 .. 2^30, row 3 zero; the even rows of W1 times 2^20 and the odd ones times 2^-20
              (a hidden row sits 2^20 above and below its input row, feature by feature); W2, W3 rows times logspace(-3, 3, 256);
              b1 = -1024 in features 64 .. 95, so the rows below 2^-10 hand the next stage a whole zero k-step; with two stages and
              more, W1[:, 0] > 0 and x[5] = (-2^31, 0, ...): the whole hidden row is zero after the ReLU and the output row is the last
              bias bit for bit"""
    import torch
    from tests.gemm_instances import plain_inputs
    tag = f"sr/chain/{M}/{stages}"
    x = plain_inputs(M, 256, 256, tag + "/x")[0]
    lay = []
    for i in range(stages):
        _, w, b, _ = plain_inputs(M, 256, 256, f"{tag}/w{i}")
        lay.append([w, None if (stages == 3 and i == 1) else b, i < stages - 1])
    if family == "rows":
        x = x * _row_powers(tag, M)
        x[CHAIN_ZERO_ROW] = 0.0
        f = torch.arange(256)
        up = torch.where(f % 2 == 0, torch.tensor(2.0 ** 20), torch.tensor(2.0 ** -20)).view(256, 1)
        w1 = lay[0][0] * up
        lay[0][1] = lay[0][1].clone()
        lay[0][1][CHAIN_DEAD_BLOCK[0]:CHAIN_DEAD_BLOCK[1]] = -1024.0
        if stages >= 2:
            w1[:, 0] = (0.05 + lay[0][0][:, 0].abs()) * up[:, 0]
            x[CHAIN_DEAD_ROW] = 0.0
            x[CHAIN_DEAD_ROW, 0] = -(2.0 ** 31)
        lay[0][0] = w1
        for i in range(1, stages):
            lay[i][0] = lay[i][0] * torch.logspace(-3, 3, 256).view(256, 1)
    else:
        assert family == "plain", family
    return x, [tuple(l) for l in lay]


def proca_inputs(case, family):
    """(qkv0 [Qp T, 3 E], kd, vd [Qp, L, T, E]) on the CPU, E = 32 h.
      plain        unit normal
      sharp        q and every key times 6
      uniform      q = 0: the output is the mean of [v0; vd]
      own_state    k0 = 8 q: the first key wins
      last_key     the last dense key = 8 q
      offset       every key = c q / |q|^2 + 0.1 z per head, c = 300 sqrt(32): every score is near +300 (exp overflows without the
                   subtraction of the maximum; with it an ordinary softmax)
      v_range_*    v0 and vd times 1e6, times 1e-6, times a per-token factor from {1, 1e-3, 1e3}"""
    import torch
    Qp, L, T, h = case
    E = 32 * h
    g = _gen(f"sr/proca/{Qp}x{L}x{T}x{h}")
    qkv0 = torch.randn(Qp * T, 3 * E, generator=g)
    kd, vd = torch.randn(Qp, L, T, E, generator=g), torch.randn(Qp, L, T, E, generator=g)
    q = qkv0[:, :E].reshape(Qp, T, E)
    if family == "sharp":
        qkv0[:, :2 * E] *= 6.0
        kd = kd * 6.0
    elif family == "uniform":
        qkv0[:, :E] = 0.0
    elif family == "own_state":
        qkv0[:, E:2 * E] = 8.0 * qkv0[:, :E]
    elif family == "last_key":
        kd[:, L - 1] = 8.0 * q
    elif family == "offset":
        qh = q.reshape(Qp, T, h, 32)
        base = (300.0 * 32 ** 0.5) * qh / (qh * qh).sum(-1, keepdim=True)            # [Qp, T, h, 32]
        qkv0[:, E:2 * E] = base.reshape(Qp * T, E) + 0.1 * qkv0[:, E:2 * E]
        kd = base.reshape(Qp, 1, T, E) + 0.1 * kd
    elif family in ("v_range_1e6", "v_range_1e-6"):
        s = float(family.split("_")[-1])
        qkv0[:, 2 * E:] *= s
        vd = vd * s
    elif family == "v_range_tokens":
        fac = torch.tensor([1.0, 1e-3, 1e3])[torch.randint(0, 3, (Qp, 1 + L, T, 1), generator=g)]
        qkv0[:, 2 * E:] *= fac[:, 0].reshape(Qp * T, 1)
        vd = vd * fac[:, 1:]
    else:
        assert family == "plain", family
    return qkv0.contiguous(), kd.contiguous(), vd.contiguous()


# ---- small_linear_kernel's arithmetic in numpy (tests/test_f16x3_numerics_cpu.py: split2, exponent)
def product_np(xop, w, scale_from=None):
    """xop @ w.T as the kernel forms it: ONE scale per row from the whole row's maximum (to 2^14), two fp16 parts per operand, three
    products per k-step of 32 (smallest terms first), the fp32 accumulator rounded after each (fp64 sums of exact part products stand
    in for the matrix unit's own summation).  `scale_from` [M]: the row whose maximum sets each row's scale -- the defect the GPU
    file's measure has to see (a row scaled by a neighbour of its tile)."""
    import numpy as np
    from tests.test_f16x3_numerics_cpu import exponent, split2
    ex, ew = exponent(np.abs(xop).max(1)), exponent(np.abs(w).max(1))
    if scale_from is not None:
        ex = ex[scale_from]
    xh, xm = split2((xop * np.exp2(14.0 - ex)[:, None].astype(np.float32)).astype(np.float32))      # exact: powers of two
    wh, wm = split2((w * np.exp2(14.0 - ew)[:, None].astype(np.float32)).astype(np.float32))
    acc = np.zeros((xop.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, xop.shape[1], 32):
        k = slice(k0, k0 + 32)
        for a, b in ((wm, xh), (wh, xm), (wh, xh)):
            acc = (acc.astype(np.float64) + b[:, k].astype(np.float64) @ a[:, k].T.astype(np.float64)).astype(np.float32)
    sx_inv, winv = np.exp2(ex - 14.0).astype(np.float32), np.exp2(ew - 14.0).astype(np.float32)
    return (acc * sx_inv[:, None]) * winv[None, :]


def operands_np(c, t):
    """(the fp32 operand of every output feature side: [(first feature, end, operand)], W[rows], b[rows]) as numpy arrays"""
    import numpy as np
    f_off, N = feature_range(c)
    x = t["x"].numpy()
    w, b = t["w"].numpy()[f_off:f_off + N], t["b"].numpy()[f_off:f_off + N]
    if t["xa"] is None:
        return [(0, N, x)], w, b
    xs = (x + t["xa"].numpy()).astype(np.float32)
    af = c["add_features"]
    return ([(0, N, xs)] if af == 0 else [(0, af, xs), (af, N, x)]), w, b


def small_linear_np(c, t, scale_from=None):
    """(y, the product alone, fp64 reference, scale = |operand| |W|^T + |b| + |residual|) of a case without LayerNorm"""
    import numpy as np
    sides, w, b = operands_np(c, t)
    M, N = c["M"], w.shape[0]
    prod, ref, scale = np.zeros((M, N), np.float32), np.zeros((M, N)), np.zeros((M, N))
    for lo, hi, xop in sides:
        prod[:, lo:hi] = product_np(xop, w[lo:hi], scale_from)
        ref[:, lo:hi] = xop.astype(np.float64) @ w[lo:hi].T.astype(np.float64)
        scale[:, lo:hi] = np.abs(xop).astype(np.float64) @ np.abs(w[lo:hi]).T.astype(np.float64)
    y = (prod + b[None]).astype(np.float32)
    ref, scale = ref + b[None].astype(np.float64), scale + np.abs(b)[None]
    if c["relu"]:
        y, ref = np.maximum(y, np.float32(0)), np.maximum(ref, 0.0)
    if t["r"] is not None:
        r = t["r"].numpy()
        y, ref, scale = (y + r).astype(np.float32), ref + r.astype(np.float64), scale + np.abs(r)
    return y, prod, ref, scale
