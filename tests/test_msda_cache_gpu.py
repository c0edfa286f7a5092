"""The per-geometry table caches of the LDS-tiled MSDA kernels (csrc/msda_geometry.h: GeoCache) run past their capacity: many
resolutions in one process, as an image dataset produces them.  A geometry is used, then more further geometries than its cache
holds (24 for the heads and strips kernels, least recently used first; 32 for msda_tiled2, oldest first), then the first again:
its tables were retired -- freed behind the events of the launches that read them -- and are built anew, and every result on
the way is right.  References: oracle/msda_torch.py in fp64 on the sampling locations and softmax weights of the reference's
sequence (ms_deform_attn.py:100-116), computed in fp32 as the reference does."""
import pytest
import torch

from oracle import msda_torch
from univs_amd import ops, synth

pytestmark = pytest.mark.gpu

M, D, P = 2, 32, 4
TOL = 3e-5          # tests/test_ops_gpu.py::test_msda_heads_matches_reference_sequence against its reference


def _level_start(shapes):
    lsi, s = [], 0
    for h, w in shapes:
        lsi.append(s)
        s += h * w
    return lsi, s


def _ref_points(shapes):
    """[1, S, 2]: pixel centres of the query's own level."""
    refs = []
    for h, w in shapes:
        ys = (torch.arange(h, dtype=torch.float32) + 0.5) / h
        xs = (torch.arange(w, dtype=torch.float32) + 0.5) / w
        yy, xx = torch.meshgrid(ys, xs, indexing="ij")
        refs.append(torch.stack([xx.reshape(-1), yy.reshape(-1)], -1))
    return torch.cat(refs, 0).unsqueeze(0)


def _operands(tag, shapes):
    """Seeded operands of one geometry (N = 1): value, raw projections (offsets in pixels of the target level, std 2; logits),
    and the reference's sampling locations / attention weights with the fp64 result they give."""
    L = len(shapes)
    lsi, S = _level_start(shapes)
    name = f"msda_cache/{tag}/" + "x".join(f"{h}.{w}" for h, w in shapes)
    value = synth.normal(name + "/value", (1, S, M, D))
    off = synth.normal(name + "/off", (1, S, M, L, P, 2), std=2.0)
    logits = synth.normal(name + "/logits", (1, S, M, L * P), std=1.5)
    ref = _ref_points(shapes)
    norm = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32).view(1, 1, 1, L, 1, 2)
    loc = ref.view(1, S, 1, 1, 1, 2) + off / norm
    attn = torch.softmax(logits, -1).view(1, S, M, L, P)
    want = msda_torch.forward(value.double(), shapes, loc.double(), attn.double()).float()
    proj = torch.cat([off.reshape(1, S, -1), logits.reshape(1, S, -1)], -1).contiguous()
    return dict(shapes=shapes, lsi=lsi, value=value, proj=proj, n_off=M * L * P * 2, ref=ref, loc=loc, attn=attn, want=want)


def _head_major_round(cuda, tag, pack, forward, generation, further):
    """Geometry A, `further` other single-level geometries, A again: every result against the reference; returns A's two."""
    results = []
    for shapes in [[(4, 6)]] + [[(4, 7 + i)] for i in range(further)] + [[(4, 6)]]:
        o = _operands(tag, shapes)
        vhm, qhm = pack(o["value"].to(cuda), o["proj"].to(cuda), o["n_off"], shapes, P)
        got = forward(vhm, qhm, o["ref"].to(cuda), shapes, o["lsi"], M, P)
        assert got is not None and ops.msda_last_tiled_generation() == generation, shapes
        err = (got.cpu() - o["want"]).abs().max().item()
        assert err < TOL, (shapes, err)
        results.append(got)
    assert len(results) == further + 2
    return results[0], results[-1]


def test_heads_cache_past_capacity(cuda):
    first, again = _head_major_round(cuda, "heads", ops.msda_pack_heads, ops.msda_forward_heads, 6, further=25)
    assert torch.equal(first, again)      # run to run bit-identical (test_msda_heads_cfg2_and_cfg5_size)


def test_strips_cache_past_capacity(cuda):
    """Generation 5 is not held to bit identity between two launches: the query slots that pad a tile repeat its last query in
    lanes with another corner order and store too, so that query's sums may round differently from launch to launch.  The bound
    is the one test_msda_strips_cfg2_and_cfg5_size puts on its second launch on a geometry (1e-5): outputs are at most 4 in
    magnitude here (weights sum to 1, values within 4 sigma), so an fp32 rounding of a partial sum is at most 2.4e-7, and an order of
    the 16 products of a single-level output makes at most 16 of them beside those it shares with another order: two orders
    differ by less than 2 * 16 * 2.4e-7 = 7.7e-6."""
    first, again = _head_major_round(cuda, "strips", ops.msda_pack_head_major, ops.msda_forward_strips, 5, further=25)
    assert (first - again).abs().max().item() < 1e-5


def test_tiled2_cache_past_capacity(cuda):
    """msda_tiled2 (generation 2) needs three levels; the smallest pyramids it covers: 2 x 2, 3 x 3 and a third level of four
    rows whose width tells the 34 geometries apart."""
    geoms = [[(2, 2), (3, 3), (4, 4 + i)] for i in range(34)]
    results = []
    with ops.configured(msda_impl=2):
        for shapes in geoms + geoms[:1]:
            o = _operands("tiled2", shapes)
            got = ops.ms_deform_attn_forward(o["value"].to(cuda), shapes, o["lsi"], o["loc"].to(cuda), o["attn"].to(cuda))
            assert ops.msda_last_impl() == 2 and ops.msda_last_tiled_generation() == 2, shapes
            err = (got.cpu() - o["want"]).abs().max().item()
            assert err < TOL, (shapes, err)
            results.append(got)
    assert len(results) == 35
    assert torch.equal(results[0], results[-1])
