"""CPU (hipcc cross-compiles gfx950 without a GPU): properties of the COMPILED attention cores (csrc/cross_attn.hip, csrc/window_attn_f16.hip)
that their instruction diet rests on and that a source edit or a compiler update can silently lose:
  * the fp16 two-part split is the two-instruction form (v_fma_mix{lo,hi}_f16, f16x3.h: l3_split2): no convert-back (v_cvt_f32_f16, the
    mark of the cvt / cvt-back / sub / cvt chain hipcc makes of the plain expression) is left in any three-product kernel, and one 32-key
    iteration of xattn_partial<NQB> splits exactly its 16 K, 16 V and 8 NQB probability values per lane;
  * no instantiation the launchers can reach uses scratch or spills a register;
  * every instantiation keeps at least the occupancy the launch choice (xa_plan: two waves per SIMD) and the window launcher count on.
The listing is made the way tests/test_isa_cpu.py makes the GEMMs'."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "univs_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")

sys.path.insert(0, os.path.join(ROOT, "tools"))
try:
    import attn_isa_count
finally:
    sys.path.pop(0)

XA_MAX_NQB = 7                                                  # csrc/cross_attn.hip
USAGE_KEYS = ("VGPRs", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")


def listing(tmp_path_factory, source):
    out = tmp_path_factory.mktemp("isa") / (source + ".s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
           os.path.join(CSRC, source), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key in USAGE_KEYS:
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                usage[name][key] = int(m.group(1))
    return attn_isa_count.bodies(str(out)), usage


@pytest.fixture(scope="module")
def cross(tmp_path_factory):
    return listing(tmp_path_factory, "cross_attn.hip")


@pytest.fixture(scope="module")
def window(tmp_path_factory):
    return listing(tmp_path_factory, "window_attn_f16.hip")


def partial_name(usage, nqb):
    return next(n for n in usage if f"xattn_partialILi{nqb}E" in n)


def window_terms(name):
    """(NB, MASK4, TERMS, NWV) of a mangled window_attn_img_f16 instantiation"""
    m = re.search(r"window_attn_img_f16ILi(\d+)ELb(\d)ELi(\d+)ELi(\d+)E", name)
    return tuple(int(x) for x in m.groups())


def test_the_instantiations_are_the_ones_the_launchers_reach(cross, window):
    _, usage = cross
    got = sorted(int(re.search(r"xattn_partialILi(\d+)E", n).group(1)) for n in usage if "xattn_partial" in n)
    assert got == list(range(1, XA_MAX_NQB + 1)), got           # (eight query blocks per wave do not fit the register file: never launched)
    _, wusage = window
    assert sorted(window_terms(n) for n in wusage if "window_attn_img_f16" in n) == sorted(
        [(4, 0, 3, 8), (4, 0, 3, 12), (6, 0, 3, 8), (9, 1, 3, 4), (9, 0, 3, 4), (4, 0, 1, 8), (6, 0, 1, 8), (9, 1, 1, 8), (9, 0, 1, 8)])


def test_no_scratch_and_no_spill_in_any_instantiation(cross, window):
    for _, usage in (cross, window):
        assert usage
        for name, u in usage.items():
            assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (name, u)


def test_occupancy_is_not_below_what_the_launchers_count_on(cross, window):
    _, usage = cross
    for nqb in range(1, XA_MAX_NQB + 1):
        want = 4 if nqb == 1 else 3 if nqb <= 3 else 2
        assert usage[partial_name(usage, nqb)]["Occupancy [waves/SIMD]"] >= want, (nqb, usage[partial_name(usage, nqb)])
    _, wusage = window
    name = next(n for n in wusage if "window_attn_img_f16" in n and window_terms(n) == (4, 0, 3, 12))
    assert wusage[name]["VGPRs"] <= 168 and wusage[name]["Occupancy [waves/SIMD]"] >= 3, wusage[name]   # twelve waves = three per SIMD


def test_no_convert_back_in_the_three_product_kernels(cross, window):
    bodies, usage = cross
    for nqb in range(1, XA_MAX_NQB + 1):
        body = bodies[partial_name(usage, nqb)]
        assert sum(l.startswith("v_mfma_f32_16x16x32_f16") for l in body) >= 12 * nqb      # (the body is the kernel's)
        assert not [l for l in body if l.startswith("v_cvt_f32_f16")], nqb
    wbodies, wusage = window
    three = [n for n in wusage if "window_attn_img_f16" in n and window_terms(n)[2] == 3]
    assert len(three) == 5
    for name in three:
        assert sum(l.startswith("v_mfma") for l in wbodies[name]) >= 9 * window_terms(name)[0]
        assert not [l for l in wbodies[name] if l.startswith("v_cvt_f32_f16")], name


@pytest.mark.parametrize("nqb", range(1, XA_MAX_NQB + 1))
def test_one_iteration_splits_each_value_with_two_mixed_precision_fmas(cross, nqb):
    bodies, usage = cross
    body = bodies[partial_name(usage, nqb)]
    loop = attn_isa_count.in_loop_lines(body, attn_isa_count.main_loop(body))                # the 32-key iteration
    assert sum(l.startswith("v_mfma_f32_16x16x32_f16") for l in loop) == 12 * nqb          # three products, two score and two output tiles per block
    mix = sum(l.startswith("v_fma_mixlo_f16") or l.startswith("v_fma_mixhi_f16") for l in loop)
    assert mix == 2 * (32 + 8 * nqb), mix                       # 16 K + 16 V + 8 NQB probabilities per lane, two instructions per value
