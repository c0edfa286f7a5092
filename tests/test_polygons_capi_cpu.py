"""CPU: the nineteenth header of the C ABI (include/univs_polygons_hip.h): its symbol is exported and bound, it shares no symbol with the
other tables, the entry answers invalid, NULL, uncovered and nothing-to-do calls before any launch, and the wrappers refuse a CPU device
with the standard sentence, after the host's own refusals."""
import ctypes
import os
import re

import pytest

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, ops, polygon_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "univs_polygons_to_runs"


def test_header_symbol_is_exported_and_bound():
    build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "univs_polygons_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text))) == [ENTRY] == sorted(_lib.POLYGONS_BINDING)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), ENTRY)
    res, args = _lib.POLYGONS_BINDING[ENTRY]
    fn = getattr(_lib.load(), ENTRY)
    assert fn.restype is res and list(fn.argtypes) == args
    assert signature_lines(_lib.POLYGONS_BINDING) == [ENTRY + " I PPPPPLIILPPPPP"]
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES")] + [_lib.IMAGELABELS_BINDING, _lib.TEXT_BINDING]
    assert len(others) == 18 and not any(set(_lib.POLYGONS_BINDING) & set(t) for t in others)
    assert "polygon_runs.hip" in build.SOURCES
    assert any(h.endswith("univs_polygons_hip.h") for h in build.HEADERS) and any(h.endswith("polygon_core.h") for h in build.HEADERS)


def test_it_is_the_nineteenth_header():
    assert len([f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")]) == 19


@pytest.fixture
def host():
    """A host buffer's address: never read, the entry answers before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


POINTERS = ("xy", "poly_start", "obj_start", "size", "slot", "bounds", "ones", "count", "status")


def _entry(p, n_points, P, N, cap_total, null=()):
    a = {k: (None if k in null else p) for k in POINTERS}
    return getattr(_lib.load(), ENTRY)(a["xy"], a["poly_start"], a["obj_start"], a["size"], a["slot"], n_points, P, N, cap_total, a["bounds"],
                                       a["ones"], a["count"], a["status"], None)


@pytest.mark.parametrize("args", [(-1, 1, 1, 8), (3, -1, 1, 8), (3, 1, -1, 8), (3, 1, 1, -8)])
def test_bad_arguments_are_invalid(host, args):
    assert _entry(host, *args) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().univs_last_error().decode() == ENTRY + ": bad arguments n_points=%d P=%d N=%d cap_total=%d" % args


@pytest.mark.parametrize("null", POINTERS)
def test_null_pointers_are_invalid(host, null):
    assert _entry(host, 3, 1, 1, 8, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().univs_last_error().decode() == ENTRY + ": NULL data pointer"


@pytest.mark.parametrize("args", [(2 ** 31, 1, 1, 8), (3, 1, 1, 2 ** 31)])
def test_beyond_each_bound_the_entry_answers_not_implemented_before_any_launch(host, args):
    assert _entry(host, *args) == _lib.ERR_NOT_IMPLEMENTED, args
    assert _lib.load().univs_last_error().decode() == ENTRY + ": not covered (n_points < 2^31, cap_total < 2^31)"


def test_nothing_to_do_is_success_without_a_launch():
    assert _entry(None, 0, 0, 0, 0) == _lib.OK and _entry(None, 5, 2, 0, 9) == _lib.OK


def test_wrappers_refuse_a_cpu_device_after_the_hosts_own_refusals():
    square = [[1, 1, 5, 1, 5, 5, 1, 5]]
    with pytest.raises(RuntimeError) as e:
        polygon_ops.polygons_to_runs([square], [(7, 7)], "cpu")
    assert str(e.value) == str(ops._cpu_refusal("polygons_to_runs", "device cpu"))
    with pytest.raises(ValueError, match="object 0, polygon 0: .*odd count"):
        polygon_ops.polygons_to_runs([[[1, 1, 5, 1, 5]]], [(7, 7)], "cpu")           # (the polygon is looked at first)
    with pytest.raises(ValueError, match="object 0: an image of 0 x 7"):
        polygon_ops.polygons_to_runs([square], [(0, 7)], "cpu")
    assert not hasattr(ops, "polygons_to_runs")                                    # (ops.py's public set is pinned)
    r = polygon_ops.polygons_to_runs_else_host([square, None], [(7, 7), (3, 3)], "cpu")
    assert r.bounds.tolist() == [8, 12, 15, 19, 22, 26, 29, 33, 49] and r.starts.tolist() == [0, 9, 9] and r.ones.tolist()[-1] == 16


def test_segmentations_of_three_kinds_make_one_runs():
    square = [[1, 1, 5, 1, 5, 5, 1, 5]]
    segms = [square, {"size": [3, 3], "counts": [2, 3, 4]}, None, {"size": [7, 7], "counts": [8, 4, 3, 4, 3, 4, 3, 4, 16]}, {"size": [3, 3], "counts": [0, 9]}]
    sizes = [(7, 7), (3, 3), (5, 5), (7, 7), (3, 3)]
    r = polygon_ops.runs_from_segmentations(segms, sizes, "cpu")
    assert r.starts.tolist() == [0, 9, 12, 12, 21, 23]
    assert r.bounds.tolist() == [8, 12, 15, 19, 22, 26, 29, 33, 49, 2, 5, 9, 8, 12, 15, 19, 22, 26, 29, 33, 49, 0, 9]
    assert r.areas().tolist() == [16, 3, 0, 16, 9]
    s = polygon_ops.slice_runs(r, 3, 5)
    assert s.starts.tolist() == [0, 9, 11] and s.bounds.tolist() == r.bounds.tolist()[12:] and s.areas().tolist() == [16, 9]
    with pytest.raises(ValueError, match="image 4: a mask of size \\[3, 3\\] on an image of \\[3, 4\\]"):
        polygon_ops.runs_from_segmentations(segms, sizes[:4] + [(3, 4)], "cpu", names=[f"image {i}" for i in range(5)])


def test_the_kernel_is_compiled_without_contraction(tmp_path):
    """The promise is the pragma at the head of csrc/polygon_core.h (build.SOURCE_FLAGS stays what the HOTA kernel's test pins): the
    device code is the same instruction for instruction with -ffp-contract=off on the command line, and another without the pragma (so
    the comparison can tell)."""
    import subprocess
    src = os.path.join(ROOT, "univs_amd", "csrc", "polygon_runs.hip")

    def instructions(name, *extra, source=src):
        out = str(tmp_path / name)
        subprocess.run([build._hipcc(), *build._flags(), "--offload-device-only", "-S", *extra, source, "-o", out], check=True, capture_output=True)
        return [line.split(";")[0].strip() for line in open(out) if re.match(r"\s+[vs]_", line)]

    plain = instructions("plain.s")
    assert plain == instructions("off.s", "-ffp-contract=off") and any(i.startswith("v_mul_f64") for i in plain)
    fused = str(tmp_path / "polygon_runs.hip")                           # the same two files without the pragma: the default contracts
    core = open(os.path.join(os.path.dirname(src), "polygon_core.h")).read()
    assert core.count("#pragma clang fp contract(off)") == 1
    open(str(tmp_path / "polygon_core.h"), "w").write(core.replace("#pragma clang fp contract(off)", ""))
    open(fused, "w").write(open(src).read())
    assert plain != instructions("fused.s", "-I", os.path.dirname(src), source=fused)
