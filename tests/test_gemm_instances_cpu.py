"""CPU: the case table of tests/gemm_instances.py -- one GPU case per compiled kernel of the three-product GEMM family.
  a. every case's plan (tools/gemm_instances_dump.cpp over csrc/gemm_plan.h, hipcc's host compiler) is the instantiation the case
     names, at 64, 256 and 304 CUs: the GPU file does not depend on the card's CU count;
  b. the kernels of the family in the BUILT library (symbol names only; template arguments read from the mangled name) are exactly
     cases + UNREACHABLE + TIMING_ONLY: a new instantiation fails here until it gets a case;
  c. the kernels the recorded GPU run launched (profiles/gemm_instances_trace_v1.txt) include every case's;
  d. the bound of the moving-scale checks holds for the reference arithmetic alone (the numpy restatement of
     tests/test_f16x3_numerics_cpu.py on the GPU file's own input generator)."""
import collections
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import gemm_instances as gi
from tests.test_f16x3_numerics_cpu import gemm_f16x3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ("linear_f16x3", "linear_bf16x6", "gemm_f16x3_stream", "gemm_f16x3_tile", "mlp_f16x3", "mlp_f16x3_ps")
TRACE = os.path.join(ROOT, "profiles", "gemm_instances_trace_v1.txt")


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


def instantiation(symbol):
    """`_ZN5univs12linear_f16x3ILi5ELi3ELb1EEEv...` -> `linear_f16x3<5,3,1>` (None for anything that is no kernel of the family).  The
    streamed kernel's trailing AFF argument is dropped where false, as tools/gemm_plan_dump.cpp prints it."""
    m = re.match(r"_ZN5univs\d+(" + "|".join(FAMILY) + r")I((?:L[ib]\d+E)+)E", symbol)
    if not m:
        return None
    args = re.findall(r"L[ib](\d+)E", m.group(2))
    if m.group(1) == "gemm_f16x3_stream" and args[-1] == "0":
        args = args[:-1]
    return f"{m.group(1)}<{','.join(args)}>"


def test_the_table_has_one_case_per_kernel_and_three_disjoint_lists():
    names = [c["inst"] for c in gi.CASES]
    assert len(set(names)) == len(names) and len({c["id"] for c in gi.CASES}) == len(names)
    assert not set(names) & set(gi.UNREACHABLE) and not set(names) & set(gi.TIMING_ONLY) and not set(gi.UNREACHABLE) & set(gi.TIMING_ONLY)
    per = collections.Counter(n.split("<")[0] for n in names)
    assert per == {"linear_f16x3": 32, "linear_bf16x6": 91, "gemm_f16x3_stream": 66, "gemm_f16x3_tile": 29, "mlp_f16x3": 10, "mlp_f16x3_ps": 6}, per
    assert instantiation("_ZN5univs12linear_f16x3ILi5ELi3ELb1EEEvPKfS2_S2_S2_Pfiiiiiiiis2_") == "linear_f16x3<5,3,1>"
    assert instantiation("_ZN5univs17gemm_f16x3_streamILi1ELi3ELi2ELb0EEEvNS_6GsArgsE") == "gemm_f16x3_stream<1,3,2>"
    assert instantiation("_ZN5univs17gemm_f16x3_streamILi1ELi3ELi2ELb1EEEvNS_6GsArgsE") == "gemm_f16x3_stream<1,3,2,1>"
    assert instantiation("_ZN5univs12mlp_f16x3_psILi8ELi2EEEvNS_7MlpArgsE") == "mlp_f16x3_ps<8,2>"
    assert instantiation("_ZN5univs18vis_overlap_kernelEPKiS1_S1_S1_S1_iiiiiPi") is None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_every_case_selects_the_instantiation_it_names_at_64_256_and_304_cus(tmp_path):
    exe = str(tmp_path / "gemm_instances_dump")
    subprocess.run([_hipcc(), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "gemm_instances_dump.cpp"),
                    "-o", exe], check=True, capture_output=True, timeout=300)
    lines = "".join(gi.plan_line(c) + "\n" for c in gi.CASES)
    out = subprocess.run([exe], input=lines, check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    got = collections.defaultdict(dict)
    for l in out:
        cid, n_cu, inst = l.split(" ", 2)
        got[cid][int(n_cu)] = inst
    wrong = [(c["id"], c["inst"], got[c["id"]]) for c in gi.CASES if got[c["id"]] != {64: c["inst"], 256: c["inst"], 304: c["inst"]}]
    assert not wrong, "cases whose plan is another kernel (id, named, planned per CU count):\n" + "\n".join(map(str, wrong[:20]))


def _compiled_kernels(tmp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_scan
    finally:
        sys.path.pop(0)
    objdump = os.path.join(isa_scan.LLVM, "llvm-objdump")
    if not os.path.exists(objdump) or shutil.which("objcopy") is None:
        pytest.skip("llvm-objdump / objcopy not found")
    from univs_amd import build
    lib = build.build()                                            # (a no-op when the binary is newer than the sources)
    found = set()
    for i, co in enumerate(isa_scan.code_objects(lib)):
        path = os.path.join(tmp, f"{i}.co")
        with open(path, "wb") as f:
            f.write(co)
        syms = subprocess.run([objdump, "--syms", path], capture_output=True, text=True, check=True).stdout
        for l in syms.splitlines():
            name = l.split()[-1] if l.split() else ""
            if name.startswith("_ZN5univs") and "." not in name:   # (the kernel itself: `.kd`, `.num_vgpr`, ... are its descriptors)
                inst = instantiation(name)
                if inst:
                    found.add(inst)
    return found


def test_the_table_is_complete_against_the_built_library(tmp_path):
    compiled = _compiled_kernels(str(tmp_path))
    listed = {c["inst"] for c in gi.CASES} | set(gi.UNREACHABLE) | set(gi.TIMING_ONLY)
    assert len(compiled) > 200, len(compiled)
    orphans, stale = sorted(compiled - listed), sorted(listed - compiled)
    assert not orphans, f"compiled kernels without a case in tests/gemm_instances.py: {orphans}"
    assert not stale, f"tests/gemm_instances.py lists kernels the library does not hold: {stale}"


def test_the_recorded_gpu_run_launched_every_case_s_kernel():
    """profiles/gemm_instances_trace_v1.txt: the family's kernel names and call counts of one run of tests/test_gemm_instances_gpu.py
    under `rocprofv3 --kernel-trace --stats`"""
    ran = set()
    with open(TRACE) as f:
        for l in f:
            if l.strip() and not l.startswith("#"):
                ran.add(l.split()[0])
    missing = [c["inst"] for c in gi.CASES if c["inst"] not in ran]
    assert not missing, f"cases whose kernel the recorded run did not launch: {missing}"
    assert not ran & (set(gi.TIMING_ONLY) | set(gi.UNREACHABLE)), sorted(ran & (set(gi.TIMING_ONLY) | set(gi.UNREACHABLE)))


@pytest.mark.parametrize("K", [96, 192, 256, 384, 768, 1152])
def test_the_moving_scale_bound_holds_for_the_reference_arithmetic(K):
    """e3 < max(4 e32, 3e-7) -- the GPU file's bound -- for the numpy restatement of the kernels' arithmetic on the GPU file's own inputs:
    the factor 4 is test_linear_fused_matches_torch's, the floor the per-product bound 2^-21.7 of linear_f16x3.hip.  One dropped part
    product (2^-12) misses it by three orders of magnitude."""
    M, N = 96, 44
    x, w, b, _ = (t.numpy() for t in gi.moving_scale_inputs(M, K, N, "cpu"))
    rec = {}
    y = gemm_f16x3(x, w, record=rec).astype(np.float64) + b.astype(np.float64)[None]
    assert rec["resets"][::2].min() >= 3                          # the rising rows lowered their scale several times
    ref = x.astype(np.float64) @ w.T.astype(np.float64) + b.astype(np.float64)[None]
    scale = np.abs(x).astype(np.float64) @ np.abs(w).T.astype(np.float64) + np.abs(b).astype(np.float64)[None] + 1e-300
    y32 = (x @ w.T + b[None]).astype(np.float64)
    e3, e32 = (np.abs(y - ref) / scale).max(), (np.abs(y32 - ref) / scale).max()
    print(f"K={K}: e3 {e3:.2e} e32 {e32:.2e}")
    assert e3 < max(4.0 * e32, 3e-7), (e3, e32)
    # ... and would catch a kernel that drops the m * h' product
    ew = np.floor(np.log2(np.abs(w).max(1)))
    w_h_only = (w * np.exp2(14 - ew)[:, None]).astype(np.float16).astype(np.float64) * np.exp2(ew - 14)[:, None]
    dropped = (x.astype(np.float64) @ w_h_only.T + b[None].astype(np.float64))
    e_dropped = (np.abs(dropped - ref) / scale).max()
    print(f"      without W's low part: {e_dropped:.2e}")
    assert e_dropped > 10 * max(4.0 * e32, 3e-7), e_dropped
