"""GPU: linear_f16x3, linear_pair_f16x3 and gemm_f16x3_stream return the bits of the commit before their k-step moved into
csrc/f16x3_kstep.h (tests/golden/gemm_parent_bits.json, written by tools/record_gemm_bits.py with that commit's library: SHA-256 of the
outputs for seeded inputs; the cases are defined in that file).

The shared functions hold the text the three kernels carried -- the same k order, running row scale, split and product order -- so
nothing may move: every instantiation of the two templated kernels on the shape and inputs of its tests/gemm_instances.py case (plain,
and moving-scale where the kernel carries a row scale), and both outputs of the pair kernel on the shapes of
tests/test_encoder_pair_gpu.py."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import record_gemm_bits as bits
finally:
    sys.path.pop(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "gemm_parent_bits.json")) as f:
        return json.load(f)


def test_the_record_holds_every_case(golden):
    assert sorted(golden) == sorted([*bits.INSTANCE_CASES, *bits.PAIR_CASES])
    kernels = {c["inst"] for c, _ in bits.INSTANCE_CASES.values()}
    assert len(kernels) == 32 + 66                  # every linear_f16x3<RB, ring, PRE> and gemm_f16x3_stream<RB, ring, XMODE[, 1]> built
    assert len(bits.PAIR_CASES) == 8


@pytest.mark.parametrize("name", [*bits.INSTANCE_CASES, *bits.PAIR_CASES])
def test_the_bits_are_the_parents(cuda, golden, name):
    if name in bits.PAIR_CASES:
        shape, o = bits.PAIR_CASES[name]
        got = bits.run_pair(shape, cuda)[o]
    else:
        got = bits.run_instance(name, cuda)
    assert bits.digest(got) == golden[name]
