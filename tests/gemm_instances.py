"""One GPU case per COMPILED kernel of the three-product GEMM family (csrc/linear_f16x3.hip, linear_split.hip: linear_bf16x6,
gemm_f16x3_stream.hip, gemm_f16x3_tile.hip, mlp_f16x3.hip).  A plain module like tests/cases.py, read by
tests/test_gemm_instances_cpu.py (the table selects what it says, at 64 / 256 / 304 CUs; it is complete against the built library)
and tests/test_gemm_instances_gpu.py (every case against fp64).

A case names the public wrapper (`call`), the shape, the epilogue, the `switches.override(...)` and `ops.configured(...)` settings
that route it, and the instantiation it is there to run, written as tools/gemm_plan_dump.cpp prints it (`linear_f16x3<5,3,1>`;
the streamed kernel with the operand affine carries a fourth argument, `gemm_f16x3_stream<2,4,1,1>`; the MLP kernels are
`mlp_f16x3<KS1,CT,ACT,NW,ABL,DB>` and `mlp_f16x3_ps<KS1,ACT>`, ACT 1 = ReLU, 2 = GELU).

Shapes are the smallest that select the kernel and still hold what goes wrong in such kernels:
  * M = 2049 (or a few rows past the bound the route needs): one row past a multiple of the 32-row tile;
  * N = 32 RB - 20 with `linear_rows_per_pass` = 16 RB: two passes of 16 RB - 8 and 16 RB - 12 features, so the last pass is short and
    its last 16-feature block holds 4 (N % 16 = 12); RB = 1: one pass of 12.  linear_bf16x6 takes no such setting: its N is picked
    per (RB, K) from its own cap (two passes where the cap allows, else one pass of 16 RB - 4);
  * K = 192 (ring of three) / 256 (ring of four): two ring groups; the tiled kernel's K = 384 is three groups of four load slots.
    linear_bf16x6<6..7,0,4,*> exist only at K = 128 (one group): wider K caps the pass below 6 blocks;
  * convolutions: T = 2 frames of 41 x 51 (H W = 2091 is no multiple of 32: a tile straddles the frame seam), Cout = 32 RB - 16 in two
    passes of 16 RB and 16 RB - 16 (Cout % 16 == 0 is the kernel's own rule).

How to add a case: append it to the builder of its kernel below (or a new builder), run tests/test_gemm_instances_cpu.py -- it names
every compiled kernel without a case and every case whose plan is another kernel -- then the GPU file."""

EPI = {"none": 0, "relu": 1, "gelu": 2, "residual": 3, "blocked": 4}
M_ROWS = 2049
FRAMES, HH, WW = 2, 41, 51           # convolutions: M = 4182 pixels

CASES = []

# Kernels no public call reaches, with the line that makes it so
UNREACHABLE = {
    "gemm_f16x3_tile<5,4,4,1>": "csrc/gemm_plan.h plan_tile: `if (p.ct == 5 && p.rb == 4 && nslot == 4) nslot = K % 96 == 0 ? 3 : 2;` (registers)",
}

# Timing ablations (UnivsConfig.linear_ablate = 2 / 3 / 4): documented as giving WRONG results (csrc/mlp_f16x3.hip, `ABL`), never run here
TIMING_ONLY = {f"mlp_f16x3<8,1,1,8,{a},1>": "encoder FFN without MFMAs / LDS reads / weight stream" for a in (1, 2, 3)}
TIMING_ONLY.update({f"mlp_f16x3<3,2,2,4,{a},1>": "Swin stage 1 MLP without MFMAs / LDS reads / weight stream" for a in (1, 2, 3)})


def _case(inst, call, shape, epi, switches=None, config=None, **more):
    c = {"inst": inst, "call": call, "shape": tuple(shape), "epi": epi, "switches": dict(switches or {}), "config": dict(config or {})}
    c.update(more)
    c["id"] = inst.replace("<", "_").replace(">", "").replace(",", "_")
    assert all(o["id"] != c["id"] for o in CASES), c["id"]
    CASES.append(c)


def _two_short_passes(rb):
    """N for `linear_rows_per_pass` = 16 rb: see the module docstring"""
    return 12 if rb == 1 else 32 * rb - 20


def _blocked_shape(K, N):
    return (M_ROWS, K, N, M_ROWS // 3, 4)          # 3 batch elements of 683 rows, column blocks of one 16-byte store


# ---- linear_f16x3<RB, ring, PRE>: the W-resident kernel on the split image (PRE) or splitting W itself
for pre in (1, 0):
    for ring, K, epis in ((4, 256, ("none", "relu", "residual", "blocked", "gelu", "blocked", "relu", "residual")),
                          (3, 192, ("relu", "residual", "none", "gelu", "residual", "none", "gelu", "relu"))):
        for rb in range(1, 9):
            epi, N = epis[rb - 1], _two_short_passes(rb)
            _case(f"linear_f16x3<{rb},{ring},{pre}>", "linear_blocked" if epi == "blocked" else "linear_fused",
                  _blocked_shape(K, N) if epi == "blocked" else (M_ROWS, K, N), epi,
                  switches={"resident_presplit": bool(pre), "presplit_kmin": 0}, config={"linear_terms": 3, "linear_rows_per_pass": 16 * rb})


# ---- linear_bf16x6<RB, ksc, ring, epi>: six bf16 products (linear_terms = 6).  N per (K, RB): K = 256 caps a pass at 104 features, K = 192
# and 128 at 112, K = 384 at 68
def _bf16x6_n(K, rb):
    cap = {256: 104, 192: 112, 128: 112, 384: 68}[K]
    two = 32 * rb - 20
    return two if (two > cap and (two // 2 + 3) // 4 * 4 <= cap) else 16 * rb - 4


for ksc, ring in ((8, 4), (0, 4), (0, 3)):
    for rb in range(1, 8):
        K = 256 if ksc else 192 if ring == 3 else (384 if rb <= 4 else 128)
        N = _bf16x6_n(K, rb)
        for epi in ("none", "relu", "gelu", "residual") + (("blocked",) if ksc else ()):
            _case(f"linear_bf16x6<{rb},{ksc},{ring},{EPI[epi]}>", "linear_blocked" if epi == "blocked" else "linear_fused",
                  _blocked_shape(K, N) if epi == "blocked" else (M_ROWS, K, N), epi,
                  switches={"resident_presplit": False, "presplit_kmin": 0}, config={"linear_terms": 6})

# ---- gemm_f16x3_stream<RB, ring, 0>: a Linear on weights split once per tensor; K < 384 keeps the tiled kernel out
for ring, K, epis in ((4, 256, ("relu", "none", "residual", "gelu", "none", "residual", "relu", "none")),
                      (3, 192, ("residual", "gelu", "none", "relu", "residual", "none", "none", "relu"))):
    for rb in range(1, 9):
        _case(f"gemm_f16x3_stream<{rb},{ring},0>", "linear_fused", (M_ROWS, K, _two_short_passes(rb)), epis[rb - 1],
              switches={"presplit_kmin": 96}, config={"linear_terms": 3, "linear_rows_per_pass": 16 * rb})


# ---- gemm_f16x3_stream<RB, ring, 1 | 2 [, affine]>: the convolutions.  XMODE 1: an NCHW operand (ring 4: the 3 x 3 for even RB, the
# 1 x 1 for odd; ring 3: the 1 x 1 at Cin = 192); XMODE 2: a channels-last view through fused_ops.conv1x1_fused
def _conv_cout(rb):
    return 16 if rb == 1 else 32 * rb - 16


for xmode in (1, 2):
    for ring in (4, 3):
        for rb in range(1, 9):
            three = xmode == 1 and ring == 4 and rb % 2 == 0
            cin = 128 if three else 256 if ring == 4 else 192
            _case(f"gemm_f16x3_stream<{rb},{ring},{xmode}>", "conv3x3" if three else "conv1x1" if xmode == 1 else "conv1x1_fused",
                  (FRAMES, cin, _conv_cout(rb), HH, WW), "none" if three or rb % 3 == 0 else "bias",
                  switches={"presplit_kmin": 768}, config={"linear_rows_per_pass": 16 * rb}, channels_last=xmode == 2, affine=False)
    for ring in (4, 3):
        for rb in (1, 2, 3, 4, 8):
            if rb == 8 and ring == 3:
                continue                               # csrc/gemm_plan.h stream_affine_plan_covered: not built
            _case(f"gemm_f16x3_stream<{rb},{ring},{xmode},1>", "conv1x1_fused", (FRAMES, 256 if ring == 4 else 192, _conv_cout(rb), HH, WW),
                  "bias" if rb % 2 else "none", switches={"presplit_kmin": 768}, config={"linear_rows_per_pass": 16 * rb},
                  channels_last=xmode == 2, affine=True)

# ---- gemm_f16x3_tile<CT, RB, slots, occupancy>: CT by linear_grid_x, RB by linear_rows_per_pass (128 / 192 / 256) and N, the load
# slots by linear_ablate 7 / 8 / 9 at K = 384 (a multiple of 64, 96 and 128).  Two workgroups per CU need more workgroups than CUs at
# 304 CUs; the one-per-CU kernels of the same tiles need no more workgroups than CUs at 64 (M = 2049: 44 at most)
_TILE_N = {2: 140, 3: 172, 4: 204}       # rb 2: two feature tiles of 72; rb 3 / 4: one of 172 / 204.  N % 16 = 12
_TILE_EPIS = ("none", "relu", "residual", "gelu", "residual", "none", "relu", "none", "residual")
for ct in (3, 4, 5):
    for rb in (2, 3, 4):
        for slots in (2, 3, 4):
            inst = f"gemm_f16x3_tile<{ct},{rb},{slots},1>"
            if inst in UNREACHABLE:
                continue
            _case(inst, "linear_fused", (M_ROWS, 384, _TILE_N[rb]), _TILE_EPIS[(3 * (ct - 3) + (rb - 2) + slots) % 9], switches={"presplit_kmin": 96},
                  config={"linear_terms": 3, "linear_grid_x": ct, "linear_rows_per_pass": 64 * rb, "linear_ablate": slots + 5})
for (ct, rb), (M, epi) in {(3, 2): (14689, "residual"), (3, 3): (29281, "none"), (4, 2): (19585, "relu")}.items():
    _case(f"gemm_f16x3_tile<{ct},{rb},2,2>", "linear_fused", (M, 384, _TILE_N[rb]), epi, switches={"presplit_kmin": 96},
          config={"linear_terms": 3, "linear_grid_x": ct, "linear_rows_per_pass": 64 * rb})

# ---- mlp_f16x3<KS1, CT, ACT, NW, 0, DB> and the phase-shifted mlp_f16x3_ps<KS1, ACT> (linear_ablate = 10).  Hd = 160: five chunks of 32
_MLP = {96: (3, 2, 4, 1), 128: (4, 1, 8, 1), 192: (6, 1, 8, 1), 256: (8, 1, 8, 1), 384: (12, 1, 4, 0)}
for C, (ks1, ct, nw, db) in _MLP.items():
    for act in (1, 2):
        _case(f"mlp_f16x3<{ks1},{ct},{act},{nw},0,{db}>", "mlp_fused", (2100, C, 160), "relu" if act == 1 else "gelu", residual=(ks1 + act) % 2 == 0)
for C in (128, 192, 256):
    for act in (1, 2):
        _case(f"mlp_f16x3_ps<{C // 32},{act}>", "mlp_fused", (2100, C, 160), "relu" if act == 1 else "gelu", config={"linear_ablate": 10},
              residual=(C // 32 + act) % 2 == 1)

BY_ID = {c["id"]: c for c in CASES}


def plan_line(c):
    """The case as tools/gemm_instances_dump.cpp reads it.  The wrapper's own routing is restated here: ops.linear_fused takes the
    pre-split entry where 0 < presplit_kmin <= K, else the resident entry (on the split image with `resident_presplit` and three
    products)."""
    cfg, sw = c["config"], c["switches"]
    rpp, gx, abl, terms = (cfg.get(k, 0) for k in ("linear_rows_per_pass", "linear_grid_x", "linear_ablate", "linear_terms"))
    if c["call"] in ("linear_fused", "linear_blocked"):
        M, K, N = c["shape"][:3]
        br, bc = c["shape"][3:] if c["call"] == "linear_blocked" else (0, 0)
        kmin = sw.get("presplit_kmin", 768)
        if c["call"] == "linear_fused" and 0 < kmin <= K:
            return f"presplit {c['id']} {M} {N} {K} {EPI[c['epi']]} {rpp} {gx} {abl}"
        assert kmin == 0 or c["call"] == "linear_blocked", c["id"]
        pre = int(bool(sw.get("resident_presplit", True)) and terms != 6)
        return f"resident {c['id']} {M} {N} {K} {EPI[c['epi']]} {br} {bc} {pre} {terms} {rpp} {gx} {abl}"
    if c["call"] in ("conv3x3", "conv1x1", "conv1x1_fused"):
        T, Cin, Cout, H, W = c["shape"]
        assert sw.get("presplit_kmin", 768) > 0, c["id"]
        return (f"conv {c['id']} {2 if c['channels_last'] else 1} {9 if c['call'] == 'conv3x3' else 1} {T} {Cin} {Cout} {H} {W} {int(c['affine'])} "
                f"{rpp} {gx} {abl}")
    assert c["call"] == "mlp_fused", c["call"]
    M, C, Hd = c["shape"]
    return f"mlp {c['id']} {M} {C} {Hd} {EPI[c['epi']]} {abl}"


# ---- inputs shared by the GPU file and the CPU check of its bound (torch's CPU generator, seeded by the case's name and shape)
def plain_inputs(M, K, N, tag):
    """x ~ N(0, 1), w ~ N(0, 1 / K), bias ~ N(0, 1 / 4), residual ~ N(0, 1): the distributions of test_linear_fused_matches_torch"""
    import zlib
    import torch
    g = torch.Generator().manual_seed(zlib.crc32(f"{tag}/{M}x{K}x{N}".encode()))
    return (torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g) * 0.5,
            torch.randn(M, N, generator=g))


def moving_scale_inputs(M, K, N, tag):
    """The inputs on which the running row scale of the three-product kernels moves: x of `plain_inputs` times logspace(-2, 2, K) along
    k -- rising in the even rows (the scale is lowered several times on the way and the accumulators rescaled), falling in the odd
    rows -- times a power of two per row from 2^-30 .. 2^30; the rows of w times logspace(-3, 3, N)."""
    import torch
    x, w, b, r = plain_inputs(M, K, N, "ms/" + tag)
    ramp = torch.logspace(-2, 2, K)
    x = x * torch.where((torch.arange(M) % 2 == 0).view(M, 1), ramp.view(1, K), ramp.flip(0).view(1, K))
    g = torch.Generator().manual_seed(M * 1000003 + K * 1009 + N)
    rows = torch.exp2(torch.randint(-30, 31, (M, 1), generator=g).float())             # exact: a power of two
    return x * rows, w * torch.logspace(-3, 3, N).view(N, 1), b, r * rows


def carries_row_scale(c):
    """The moving-scale family: the kernels with a running row scale, epilogues none / ReLU / residual / blocked"""
    return not c["inst"].startswith("linear_bf16x6") and c["epi"] != "gelu"
