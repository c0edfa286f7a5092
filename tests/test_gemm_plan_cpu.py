"""What the three-product GEMM family launches (csrc/gemm_plan.h: coverage rules, passes, row ranges, the tile chooser's cost model)
printed on the host by tools/gemm_plan_dump.cpp -- built with hipcc's host compiler over the SAME header the launchers include -- and
compared line by line with tests/gemm_plan_table.txt: every launch of tools/gemmset.py at T = 5, the config-4 / config-5 Swin Linears,
every shape of the family's GPU tests, and the edges of each rule, at 256 CUs; the gemmset launches again at 64 CUs.  No GPU.

The table was recorded from the launchers as they stood BEFORE the planning moved into the header: their bodies copied verbatim into
a scratch program (config() and the CU query turned into parameters, the launch macro into the same print; the dump tool's
-DGEMM_PLAN_DUMP_PLANNERS hook runs such a transcription over the same cases).  Never regenerate it from the code under test: a line
that differs means a Linear of the model now runs another kernel, grid or LDS size than it was measured with.  New cases are
appended with the lines of the code as it stands before the change they are meant to guard."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "gemm_plan_table.txt")


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_launch_plans_match_the_recorded_table(tmp_path):
    exe = str(tmp_path / "gemm_plan_dump")
    subprocess.run([_hipcc(), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "gemm_plan_dump.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    got = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    with open(TABLE) as f:
        want = f.read().splitlines()
    assert len(want) > 600
    diff = [(i + 1, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, "first differing lines (line, recorded, now):\n" + "\n".join(f"{i}: {w}\n{' ' * len(str(i))}  {g}" for i, w, g in diff[:10])
    assert len(got) == len(want)
    # the table holds what it is meant to hold: every kernel of the family, both rings, every RB, both occupancies
    text = "\n".join(want)
    for rb in range(1, 9):
        assert f"linear_f16x3<{rb}," in text and f"gemm_f16x3_stream<{rb}," in text
    for rb in range(1, 8):
        assert f"linear_bf16x6<{rb}," in text
    for inst in ("gemm_f16x3_tile<3,2,2,2>", "gemm_f16x3_tile<3,2,2,1>", "gemm_f16x3_tile<5,4,3,1>", "gemm_f16x3_stream<8,4,1>", "gemm_f16x3_stream<8,4,2>",
                 "linear_bf16x6<6,8,4,4>", "linear_f16x3<8,3,1>"):
        assert inst in text, inst
    assert "grid=(15,17)" in text                               # 17 passes: 15 row ranges, not 8
    assert sum("not covered" in l for l in want) > 50


def test_the_header_is_free_of_hip():
    """csrc/gemm_plan.h is host-only by construction: no HIP include, no runtime call, no config()."""
    src = open(os.path.join(ROOT, "univs_amd", "csrc", "gemm_plan.h")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "hip" not in code.replace("univs_hip.h", "").lower() and "config()" not in code and "cu_count" not in code
