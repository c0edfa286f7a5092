"""SHA-256 of what the three-product GEMM kernels that share csrc/f16x3_kstep.h (linear_f16x3.hip, linear_pair_f16x3.hip,
gemm_f16x3_stream.hip) return for seeded inputs.

    python tools/record_gemm_bits.py [--out tests/golden/gemm_parent_bits.json]

Run on the GPU with the library of the commit whose bits are to be kept (UNIVS_HIP_LIB names another build of it); the file it
writes is what tests/test_gemm_bits_gpu.py requires of every later tree: moving the k-step of these kernels into shared functions
keeps every bit.  The cases are defined here, once; the test imports them from this file:
  * every case of tests/gemm_instances.py whose instantiation is linear_f16x3<...> or gemm_f16x3_stream<...>, on its own shape
    (M = 2049 rows, convolutions 2 x 41 x 51), built and called as tests/test_gemm_instances_gpu.py builds and calls it: the plain
    inputs, and the moving-scale inputs where `carries_row_scale(c)`;
  * the four SHAPES of tests/test_encoder_pair_gpu.py, both outputs, moving-scale inputs.
Inputs come from the seeded CPU generators of tests/gemm_instances.py, and a feature's sum depends on nothing but its row of x and
its row of W -- never on the grid -- so the record does not depend on the CU count of the box it was made on."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import gemm_instances as gi  # noqa: E402
from tests import test_encoder_pair_gpu as pair  # noqa: E402
from tests import test_gemm_instances_gpu as inst  # noqa: E402
from univs_amd import ops  # noqa: E402

KERNELS = ("linear_f16x3<", "gemm_f16x3_stream<")
# name -> (case of gemm_instances, moving-scale inputs)
INSTANCE_CASES = {f"{c['id']}/{'moving' if moving else 'plain'}": (c, moving)
                  for c in gi.CASES if c["inst"].startswith(KERNELS)
                  for moving in ((False, True) if gi.carries_row_scale(c) else (False,))}
# name -> ((T, S, N_b, column block of B), output 0 = A / 1 = B)
PAIR_CASES = {f"linear_pair_{T}x{S}x{NB}/{'AB'[o]}": ((T, S, NB, cb), o) for (T, S, NB, cb) in pair.SHAPES for o in (0, 1)}


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_instance(name, device):
    c, moving = INSTANCE_CASES[name]
    build = inst._linear if c["call"].startswith("linear") else inst._conv
    with ops.configured(linear_terms=c["config"].get("linear_terms", 3)):
        t = build(c, device, moving)[0]
        return inst.run(c, t)


def run_pair(shape, device):
    """(Ya, Yb) of one shape: one launch for both records"""
    T, S, NB, cb = shape
    with ops.configured(linear_terms=3):
        return pair._pair(pair._inputs(T, S, NB, True, device), cb)


def record(device):
    out = {name: digest(run_instance(name, device)) for name in INSTANCE_CASES}
    for shape in pair.SHAPES:
        y = run_pair(shape, device)
        out.update({name: digest(y[o]) for name, (s, o) in PAIR_CASES.items() if s == shape})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_parent_bits.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    got = record(torch.device("cuda:0"))
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for n, h in sorted(got.items()):
        print(h[:16], n)


if __name__ == "__main__":
    main()
