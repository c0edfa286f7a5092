"""CPU: the polygon rasteriser's kernel text (csrc/polygon_core.h) compiled for the host by tools/polygon_host.cpp with the address and
undefined-behaviour sanitizers and run as a child process: by the kernel's lane schedule it gives the rule's boundaries on the whole
corpus of tests/polygon_cases.py, and tables and coordinates that lie end every object with a status inside its slots.  Nothing
sanitised is loaded into Python."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import polygon_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    from univs_amd import build
    out = str(tmp_path_factory.mktemp("polygon_host") / "sanitized")
    cc = [build._hipcc(), "-x", "c++"]
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if "clang" not in subprocess.run([cc[0], "--version"], capture_output=True, text=True).stdout:
        flags += ["-static-libasan", "-static-libubsan"]
    if "hipcc" in cc[0]:
        flags = [a for f in flags for a in ("-Xarch_host", f)]
    subprocess.run([*cc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", *flags, os.path.join(ROOT, "tools", "polygon_host.cpp"), "-o", out],
                   check=True)
    return out


def _run(program, blob):
    r = subprocess.run([program], input=blob, capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    return cases.parse_host_output(r.stdout.decode())


def test_the_lane_schedule_gives_the_rule_on_the_corpus(host_program):
    objects, sizes = cases.objects_and_sizes()
    got = _run(host_program, cases.host_call(objects, sizes))
    b, ones, s = (x.numpy() for x in cases.expected())
    assert len(got) == len(objects)
    for i, (name, (status, gb, go)) in enumerate(zip(cases.names(), got)):
        if name == "above_cap":
            assert (status, gb) == (1, []), name
            continue
        assert status == 0 and gb == list(b[s[i]:s[i + 1]]) and go == list(ones[s[i]:s[i + 1]]), name


def test_too_few_slots_are_a_status_not_a_store(host_program):
    objects, sizes = [[[1, 1, 6, 1, 6, 6, 1, 6]], [[1, 1, 6, 1, 6, 6, 1, 6]], [[1, 1, 6, 1, 6, 6, 1, 6]]], [(7, 7)] * 3
    got = _run(host_program, cases.host_call(objects, sizes, slots=np.array([11, 10, 0])))      # 10 boundaries and h w
    assert [g[0] for g in got] == [0, 6, 6] and len(got[0][1]) == 11


def _raw_call(obj_start, poly_start, size, slot, xy, cap_total):
    N, P = len(obj_start) - 1, len(poly_start) - 1
    return (struct.pack("<4q", N, P, len(xy) // 2, cap_total) + np.asarray(obj_start, "<i4").tobytes() + np.asarray(poly_start, "<i4").tobytes()
            + np.asarray(size, "<i4").tobytes() + np.asarray(slot, "<i8").tobytes() + np.asarray(xy, "<f8").tobytes())


def test_tables_and_coordinates_that_lie_end_with_a_status(host_program):
    big = 2 ** 31 - 1
    square = [1.0, 1.0, 6.0, 1.0, 6.0, 6.0, 1.0, 6.0]
    xy = square + [float("nan"), 1.0, 6.0, float("inf"), 3.0, 3.0] + [1e300, -1e300, 2.0 ** 24 + 1, 0.0, 5.0, 5.0] + square
    poly_start = [0, 4, 7, 10, 14]
    calls = {
        "statuses": _raw_call([0, 1, 2, 3, 4], poly_start, [7, 7, 7, 7, 7, 7, 0, 7], [0, 20, 40, 60, 80], xy, 80),
        "wild tables": _raw_call([-5, big, 1, 9], [3, -big, big, 2, 8], [7, 7, big, big, -3, 4], [-9, big, 5, -1], xy, 64),
        "two points": _raw_call([0, 1], [0, 2], [7, 7], [0, 8], xy, 8),
        "huge edges": _raw_call([0, 1], [0, 3], [7, 7], [0, 8], [-2.0 ** 24, -2.0 ** 24, 2.0 ** 24, 2.0 ** 24, -2.0 ** 24, 2.0 ** 24], 8),
    }
    got = {k: _run(host_program, v) for k, v in calls.items()}
    assert [g[0] for g in got["statuses"]] == [0, 5, 5, 3]
    assert got["statuses"][0][1] == [8, 13, 15, 20, 22, 27, 29, 34, 36, 41, 49]
    assert all(0 <= g[0] <= 6 for g in got["wild tables"]) and len(got["wild tables"]) == 3
    assert got["two points"][0][0] == 5
    assert got["huge edges"][0][0] == 2                                  # 2^26 + 1 points: beyond the point cap, before any of them is made


def test_the_tool_and_the_kernel_compile_the_same_header():
    tool = open(os.path.join(ROOT, "tools", "polygon_host.cpp")).read()
    kernel = open(os.path.join(ROOT, "univs_amd", "csrc", "polygon_runs.hip")).read()
    assert '#include "../univs_amd/csrc/polygon_core.h"' in tool and '#include "polygon_core.h"' in kernel
    assert "pg_object<Serial>(ex" in tool and "pg_object(ex, A, (int)blockIdx.x, L)" in kernel
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "univs_amd", "csrc", "polygon_core.h")).read()
