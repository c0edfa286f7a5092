"""CPU: the routing of the 3 x 3 convolution between its two kernels (csrc/conv3x3_wide_plan.h, tools/conv3x3_wide_plan.cpp over it with
hipcc's host compiler; csrc/conv3x3_wide.hip, csrc/gemm_f16x3_stream.hip):
  * the library builds with the new source and header listed in build.SOURCES / build.HEADERS;
  * the wide kernel's coverage predicate equals its documented rule restated here in Python: what the streamed kernel covers of a 3 x 3
    (Cin % 128 == 0, Cout % 16 == 0, M >= 4096, byte offsets below 2^31) with Cout == 256;
  * its row ranges (workgroup b runs rounds b * rounds .. of the sequence of 8-tile rounds) assign every wave tile of 32 pixels to exactly
    one (workgroup, round, wave) at 64, 256 and 304 CUs -- none twice, none beyond M -- with no more workgroups than CUs, as few rounds
    per workgroup as that many CUs allow and less than one round per workgroup idle in all; its LDS fits the CU's 160 KB;
  * the plan header is free of HIP."""
import os
import shutil
import subprocess

from univs_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shapes of tests/test_conv3x3_wide_gpu.py, the config-2 clip (5 x 184 x 320) and 10 x 272 x 480, at the wide kernel's features ...
SIZES = [1 * 64 * 64, 1 * 50 * 83, 2 * 46 * 45, 3 * 37 * 41, 5 * 92 * 160, 5 * 184 * 320, 10 * 272 * 480]
CASES = [(M, cin, 256) for M in SIZES for cin in (128, 256)] + [
    (4095, 256, 256), (4096, 256, 256),                          # ... the lower edge of M
    (4150, 256, 128), (4150, 256, 16), (4150, 256, 512), (4150, 256, 240),   # other feature counts: the streamed kernel (240: no kernel)
    (4150, 64, 256), (4150, 96, 256), (4150, 384, 256), (4150, 512, 256),    # Cin % 128
    (2 ** 21 - 1, 256, 256), (2 ** 21, 256, 256),                # byte offsets beyond a buffer descriptor's range
]


def _stream_rule(M, Cin, Cout):
    """csrc/gemm_plan.h stream_conv_covered, a 3 x 3"""
    return Cin % 128 == 0 and Cout % 16 == 0 and M >= 4096 and M * max(Cin, Cout) * 4 < 2 ** 31 - 1


def _wide_rule(M, Cin, Cout):
    """csrc/conv3x3_wide_plan.h, `Covered:`"""
    return _stream_rule(M, Cin, Cout) and Cout == 256


def test_sources_are_listed_and_the_library_builds():
    assert "conv3x3_wide.hip" in build.SOURCES and any(h.endswith("conv3x3_wide_plan.h") for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, s)) for s in ("conv3x3_wide.hip", "conv3x3_wide_plan.h"))
    build.build()
    assert os.path.exists(build.LIB)


def test_coverage_equals_the_documented_rule_and_every_wave_tile_is_assigned_once(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "conv3x3_wide_plan")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "conv3x3_wide_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    run = subprocess.run([exe], input="".join(" ".join(str(v) for v in c) + "\n" for c in CASES), capture_output=True, text=True, timeout=120)
    out = [l.split() for l in run.stdout.splitlines()]
    assert run.returncode == 0 and len(out) == 3 * len(CASES), run.stdout + run.stderr
    n_wide = 0
    for case, n_cu, l in zip([c for c in CASES for _ in range(3)], [64, 256, 304] * len(CASES), out):
        M, Cin, Cout = case
        stream, wide = _stream_rule(*case), _wide_rule(*case)
        assert l[:6] == [str(M), str(Cin), str(Cout), str(n_cu), f"stream={int(stream)}", f"wide={int(wide)}"], (case, l)
        assert len(l) == (11 if wide else 6)
        if not wide:
            continue
        n_wide += 1
        nwg, rounds, lds, idle = int(l[6]), int(l[7]), int(l[8]), int(l[10].split("=")[1])
        total = -(-(-(-M // 32)) // 8)                           # rounds of 8 wave tiles in all
        assert l[9] == "once=1", (case, n_cu, l)
        assert 1 <= nwg <= n_cu and rounds == -(-total // n_cu) and nwg == -(-total // rounds), (case, n_cu, l)
        assert idle == total * 8 - (-(-M // 32)) < 8, (case, n_cu, l)   # only the last round of the last workgroup has idle waves
        assert lds == 4 * 32768 + 2 * 256 * 4 <= 160 * 1024
    assert n_wide == 3 * (2 * len(SIZES) + 4)                    # + the edge of M, Cin = 384 and 512, the last M below 2^21
    # the clip of the benchmark on the card it is measured on: 230 workgroups x 5 rounds, exact
    i = CASES.index((5 * 184 * 320, 256, 256)) * 3 + 1
    assert out[i][3] == "256" and out[i][6:8] == ["230", "5"] and out[i][10] == "idle=0"


def test_the_plan_header_is_free_of_hip():
    src = open(os.path.join(ROOT, "univs_amd", "csrc", "conv3x3_wide_plan.h")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "hip" not in code.lower() and "config()" not in code and "cu_count" not in code
