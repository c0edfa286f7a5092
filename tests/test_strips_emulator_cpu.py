"""The data flow of csrc/msda_strips.hip emulated on the host (tools/strips_emulate.cpp, built with hipcc's host compiler over the
SAME geometry header the kernel includes, csrc/msda_strips_geom.h): tile tables, entering-row lists, the circular LDS windows,
the sample record with its lane-specific corner / chunk order, the FMA division -- against an fp64 evaluation of
ms_deform_attn_forward (ops/src/cuda/ms_deform_im2col_cuda.cuh:242-304) on nine geometries incl. slices of BASELINE config 2 and 5.
No GPU: this is the part of the MSDA kernel that is host logic."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


# 64-bit FNV-1a over the raw bytes of the tables the kernel reads (lv, tiles, pieces, qtab), one per case, as built by the two
# table builders BEFORE they became one (csrc/msda_window_geom.h): the builder must keep producing these bytes.  Recorded
# once; never regenerate them from the code under test.
TABLE_DIGESTS = {
    "cfg1": "945dfa2d23b3cc40",
    "ragged": "b8576e2478ec79c1",
    "L4-fine-first": "a67cec007e69a3dd",
    "L1": "bf4672240d952623",
    "L2-tiny-halo": "30be6676f8fa2dd2",
    "two-px": "0de186ca39af1d7d",
    "cfg2-slice": "1b5d4626868a3f2f",
    "cfg2-th6": "2a58a9671c184582",
    "cfg5-slice": "bc2a3d81a3880946",
}


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_strips_data_flow_on_the_host(tmp_path):
    exe = str(tmp_path / "strips_emulate")
    subprocess.run([_hipcc(), "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "strips_emulate.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout
    rows = [l for l in out.splitlines() if "max err" in l]
    assert len(rows) >= 9 and out.strip().endswith("all ok"), out
    for l in rows:
        m = re.search(r"max err ([0-9.e+-]+), bank conflicts (\d+), stale reads (\d+), unwritten outputs (\d+), inexact divisions (\d+)", l)
        assert m, l
        assert float(m.group(1)) < 2e-5 and all(int(m.group(i)) == 0 for i in range(2, 6)), l
    assert any(l.startswith("cfg2-slice") for l in rows) and any(l.startswith("cfg5-slice") for l in rows)
    got = dict(re.match(r"tables (.+) ([0-9a-f]{16})$", l).groups() for l in out.splitlines() if l.startswith("tables "))
    assert got == TABLE_DIGESTS
