"""CPU: the second header of the C ABI (include/univs_eval_hip.h): its symbols are exported and bound, the binding read from it is the
recorded one (tests/vis_capi_signatures.txt), its entry validates without launching, and the first header's table is untouched."""
import ctypes
import os
import re

import pytest

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_eval_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ["univs_vis_overlap_counts"] == sorted(_lib.EVAL_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_eval_hip.h but not exported"
        res, args = _lib.EVAL_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signature_is_the_recorded_one():
    recorded = open(os.path.join(ROOT, "tests", "vis_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.EVAL_SIGNATURES) == recorded == ["univs_vis_overlap_counts I PPPPPIIIIIIPP"]


def test_the_first_header_keeps_its_76_symbols():
    assert len(_lib.SIGNATURES) == 76 and not set(_lib.SIGNATURES) & set(_lib.EVAL_SIGNATURES)
    assert signature_lines(_lib.SIGNATURES) == open(os.path.join(ROOT, "tests", "capi_signatures.txt")).read().splitlines()


@pytest.mark.parametrize("sizes", [(0, 1, 1, 4, 4, 2), (1, 0, 1, 4, 4, 2), (1, 1, 0, 4, 4, 2), (1, 1, 1, 0, 4, 2), (1, 1, 1, 4, -1, 2),
                                   (1, 1, 1, 4, 4, -1), (2048, 1024, 1024, 4, 4, 2)])
def test_bad_sizes_are_invalid_arguments(sizes):
    lib = _lib.load()
    buf = (ctypes.c_int * 4)()                                            # host memory: never read, the entry returns before any launch
    p = ctypes.addressof(buf)
    assert lib.univs_vis_overlap_counts(p, p, p, p, p, *sizes, p, None) == _lib.ERR_INVALID_ARGUMENT
    msg = lib.univs_last_error().decode()
    assert msg.startswith("univs_vis_overlap_counts: bad arguments") and f"D={sizes[0]} G={sizes[1]} T={sizes[2]}" in msg


@pytest.mark.parametrize("null_at", [0, 1, 2, 3, 4, 5])
def test_null_pointers_are_invalid_arguments(null_at):
    lib = _lib.load()
    buf = (ctypes.c_int * 4)()
    p = [ctypes.addressof(buf)] * 6
    p[null_at] = None
    assert lib.univs_vis_overlap_counts(*p[:5], 1, 1, 1, 4, 4, 2, p[5], None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == "univs_vis_overlap_counts: NULL data pointer"


@pytest.mark.parametrize("sizes", [(1, 1, 1, 65536, 32768, 2), (1, 1, 1, 4, 4, 16385), (1, 1, 65536, 4, 4, 2)])
def test_beyond_its_bounds_the_entry_answers_not_implemented_before_any_launch(sizes):
    lib = _lib.load()
    buf = (ctypes.c_int * 4)()
    p = ctypes.addressof(buf)
    assert lib.univs_vis_overlap_counts(p, p, p, p, p, *sizes, p, None) == _lib.ERR_NOT_IMPLEMENTED
    assert "at most 16384 boundaries per ground-truth mask" in lib.univs_last_error().decode()
