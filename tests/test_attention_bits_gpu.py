"""GPU: the attention cores return the bits of the commit before their instruction diet (tests/golden/attn_parent_bits.json, written by
tools/record_attn_bits.py with that commit's library: SHA-256 of the outputs for seeded inputs; the cases are defined in that file).

The two-instruction fp16 split, the byte-select mask tests and the hoisted bound test compute the same values as the expressions they
replace, so nothing may move.  The cross-attention cases force three key segments (the merge's order of summation is part of the
record); at a forced segment count the result must not depend on how many query blocks a wave takes either: same keys, same order, per
query.  Under the library's own (segments, query blocks) choice only the tolerance tests of tests/test_ops_gpu.py apply."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import record_attn_bits as bits
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu
XA_MAX_NQB = 7                                                  # csrc/cross_attn.hip


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "attn_parent_bits.json")) as f:
        return json.load(f)


def test_the_record_holds_every_case(golden):
    assert sorted(golden) == sorted([*bits.XATTN_CASES, *bits.WINDOW_CASES])
    assert len(bits.XATTN_CASES) == 5 and len(bits.WINDOW_CASES) == 6


@pytest.mark.parametrize("name", list(bits.XATTN_CASES))
def test_cross_attention_bits_are_the_parents(cuda, golden, name):
    assert bits.digest(bits.run_xattn(name, cuda)) == golden[name]


@pytest.mark.parametrize("name", list(bits.WINDOW_CASES))
def test_window_attention_bits_are_the_parents(cuda, golden, name):
    assert bits.digest(bits.run_window(name, cuda)) == golden[name]


@pytest.mark.parametrize("name", list(bits.XATTN_CASES))
def test_cross_attention_does_not_depend_on_the_query_blocks_per_wave(cuda, golden, name):
    """UnivsConfig.xattn_segments = segments + 65536 x (query blocks per wave) fixes both launch choices."""
    L = bits.XATTN_CASES[name][0]
    largest = min(XA_MAX_NQB, (L + 15) // 16)
    for nqb in range(1, largest + 1):                            # every xattn_partial<NQB> the case's L allows, 3 / 5 / 6 included
        got = bits.run_xattn(name, cuda, segments=bits.SEGMENTS + 65536 * nqb)
        assert bits.digest(got) == golden[name], nqb


def test_fewer_queries_give_the_same_rows(cuda):
    """... and through the library's own choice of the query blocks: L = 16, 32, 64 against the rows of the L = 100 result."""
    name = "xattn_100x920x5x8_flags"
    full = bits.run_xattn(name, cuda)
    for rows in (16, 32, 64):
        assert torch.equal(bits.run_xattn(name, cuda, rows=rows), full[:rows]), rows
