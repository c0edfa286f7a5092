"""CPU: the routing of univs_encoder_linear_pair_presplit_f32 between its two kernels (csrc/pair_xres_plan.h, tools/encoder_xres_plan.cpp
over it with hipcc's host compiler; csrc/linear_pair_xres.hip, csrc/linear_pair_f16x3.hip):
  * the library builds with the new source and header listed in build.SOURCES / build.HEADERS;
  * the x-resident kernel's coverage predicate agrees with the entry's documented rules (include/univs_encoder_hip.h) restated here in
    Python: it never takes a call the entry does not answer, and inside the entry's set it takes the calls whose feature counts are whole
    chunks of 32, at least three per problem -- the model's shape and every shape of the two GPU test files among them;
  * its walk (workgroups persistent over groups of 128 rows, 16 rows per wave, chunks of 32 features) writes every cell of both outputs
    exactly once at 64, 256 and 304 CUs, and its LDS fits;
  * what the entry does not cover is still refused before any launch, with the same sentence, whichever kernel is selected
    (UnivsConfig.linear_ablate = 11 forces the pass kernel)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests.test_encoder_pair_cpu import COVERED, NAME, _call
from univs_amd import _lib, build, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (M, N_a, N_b, K, add_rows, blk_rows, blk_cols_a, blk_cols_b)
CASES = [
    (96600, 256, 288, 256, 19320, 19320, 32, 36),        # the model's clip
    (1, 256, 288, 256, 1, 1, 32, 36), (127, 256, 288, 256, 127, 127, 32, 36), (128, 256, 96, 256, 64, 64, 32, 12),
    (129, 256, 288, 256, 43, 43, 32, 36), (273, 256, 96, 256, 91, 91, 32, 12), (33000, 256, 288, 256, 11000, 11000, 32, 36),
    (40, 256, 288, 256, 40, 40, 32, 36), (903, 256, 288, 256, 301, 301, 32, 36), (8226, 256, 288, 256, 4113, 4113, 32, 36),
    (903, 256, 96, 256, 301, 301, 32, 12),               # ... and the shapes of the two GPU test files
    (8226, 240, 288, 256, 4113, 4113, 24, 36),           # the entry's (two passes of 120 features), but 240 is no multiple of 32: the pass kernel
    (8226, 256, 180, 256, 4113, 4113, 32, 36),           # likewise B = 2 x 90
    (8227, 256, 288, 256, 4113, 4113, 32, 36),           # M % add_rows != 0
    (8226, 256, 288, 256, 2742, 4113, 32, 36),           # add_rows != rows_per_batch
    (8226, 256, 288, 128, 4113, 4113, 32, 36), (8226, 256, 288, 512, 4113, 4113, 32, 36),   # K
    (8226, 256, 288, 256, 4113, 4113, 32, 40),           # 288 is no multiple of 40
    (8226, 256, 288, 256, 4113, 4113, 32, 6),            # a block width that is no multiple of 4
    (8226, 192, 288, 256, 4113, 4113, 32, 36), (8226, 256, 256, 256, 4113, 4113, 32, 32), (8226, 256, 64, 256, 4113, 4113, 32, 32),   # passes
    (1863680 * 2, 256, 288, 256, 1863680, 1863680, 32, 36),   # byte offsets beyond a buffer descriptor's range
]


def _entry_rule(M, Na, Nb, K, add_rows, rows, ca, cb):
    """include/univs_encoder_hip.h, `Covered:` (pointers aligned)"""
    def passes(N, cap):                                    # csrc/gemm_plan.h plan_passes: as few as the cap allows, balanced, rounded up to 4
        n = -(-N // cap)
        return -(-(-(-N // n)) // 4) * 4
    return (K == 256 and add_rows == rows and M % rows == 0 and ca % 4 == 0 and cb % 4 == 0 and Na % ca == 0 and Nb % cb == 0
            and 113 <= passes(Na, 128) <= 128 and 81 <= passes(Nb, 128) <= 96 and M * max(K, Na, Nb) * 4 < 2 ** 31)


def test_sources_are_listed_and_the_library_builds():
    assert "linear_pair_xres.hip" in build.SOURCES and "linear_pair_f16x3.hip" in build.SOURCES
    assert any(h.endswith("pair_xres_plan.h") for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in ("linear_pair_xres.hip", "pair_xres_plan.h"))
    build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)


def test_coverage_agrees_with_the_documented_rules_and_every_cell_is_written_once(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "encoder_xres_plan")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "encoder_xres_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in CASES), capture_output=True, text=True, timeout=120)
    out = [l.split() for l in run.stdout.splitlines()]
    assert run.returncode == 0 and len(out) == 3 * len(CASES), run.stdout + run.stderr
    for case, n_cu, l in zip([c for c in CASES for _ in range(3)], [64, 256, 304] * len(CASES), out):
        M, Na, Nb, K = case[:4]
        entry = _entry_rule(*case)
        xres = entry and Na % 32 == 0 and Nb % 32 == 0 and min(Na, Nb) >= 96
        assert l[:7] == [str(M), str(Na), str(Nb), str(K), str(n_cu), f"entry={int(entry)}", f"xres={int(xres)}"], (case, l)
        if xres:
            grid, lds = int(l[7]), int(l[8])
            assert l[9] == "once=1" and grid == min(n_cu, -(-M // 128)) and lds == 4 * 32768 + 8 * (Na + Nb) <= 160 * 1024 - 2048
    covered = [c for c in CASES if _entry_rule(*c)]
    assert len(covered) == 13 and sum(c[1] % 32 == 0 and c[2] % 32 == 0 for c in covered) == 11


@pytest.mark.parametrize("case", [dict(M=8226 + 1), dict(K=128), dict(Na=240), dict(cb=6), dict(Nb=256, cb=32), dict(off="x"), dict(off="yb"),
                                  dict(M=2 ** 21, add_rows=2 ** 20, rows=2 ** 20)])
def test_refusals_do_not_depend_on_the_kernel_selected(case):
    buf = (ctypes.c_char * 256)()                          # a 16-byte aligned host address: never read, the entry answers before any launch
    host = (ctypes.addressof(buf) + 15) // 16 * 16
    lib = _lib.load()
    for ablate in (0, 11):
        with ops.configured(linear_ablate=ablate):
            assert _call(lib, host, **case) == _lib.ERR_NOT_IMPLEMENTED, (case, ablate)
            assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"
    del buf
