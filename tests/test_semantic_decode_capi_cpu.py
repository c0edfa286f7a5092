"""CPU: the fifth header of the C ABI (include/univs_semantic_hip.h): its symbol is exported and bound, the binding read from it is the
recorded one (tests/semantic_capi_signatures.txt), it shares no symbol with the four other tables, its entry answers invalid and uncovered
arguments before any launch, and the wrapper refuses CPU tensors with the standard sentence."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, ops, semantic_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_semantic_quality_counts_f32"
COVERED = ("not covered (ceil(T / t_step) HW < 2^31, C HW 4 < 2^31, ceil(T / t_step) <= 65535, N <= 2097120, C <= 315, or up to 1239 where few "
           "rows make a smaller LDS tile)")


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_semantic_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == [NAME] == sorted(_lib.SEMANTIC_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_semantic_hip.h but not exported"
        res, args = _lib.SEMANTIC_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "semantic_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.SEMANTIC_SIGNATURES) == recorded == [NAME + " I PPIIIIIFFPP"]
    others = set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES)
    assert not set(_lib.SEMANTIC_SIGNATURES) & others
    assert (len(_lib.SIGNATURES), len(_lib.EVAL_SIGNATURES), len(_lib.FUSED_SIGNATURES), len(_lib.PVOS_SIGNATURES)) == (76, 1, 3, 1)
    assert "semantic_decode.hip" in build.SOURCES
    assert any(h.endswith("univs_semantic_hip.h") for h in build.HEADERS) and any(h.endswith("skinny_gemm_f32.h") for h in build.HEADERS)


def _call(lib, p, T, N, C, HW, t_step, mask_embed=True, features=True, counts=True):
    return getattr(lib, NAME)(p if mask_embed else None, p if features else None, T, N, C, HW, t_step, 1.0, -1.0, p if counts else None, None)


@pytest.fixture
def host():
    """A host buffer's address: never read, the entry answers before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


@pytest.mark.parametrize("sizes", [(0, 4, 4, 4, 1), (1, 0, 4, 4, 1), (1, 4, -1, 4, 1), (1, 4, 4, 0, 1), (1, 4, 4, 4, 0), (-2, 4, 4, 4, -7)])
def test_bad_sizes_are_invalid_arguments(host, sizes):
    lib = _lib.load()
    assert _call(lib, host, *sizes) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": bad arguments T=%d N=%d C=%d HW=%d t_step=%d" % sizes


@pytest.mark.parametrize("null", ["mask_embed", "features", "counts"])
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, 2, 4, 4, 4, 1, **{null: False}) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


@pytest.mark.parametrize("sizes", [
    (4, 8, 1, 2 ** 29, 1),             # ceil(T / t_step) HW = 2^31: a count would leave an int32
    (1, 8, 256, 2 ** 21, 1),           # C HW 4 = 2^31: a frame of the features leaves a 32-bit buffer range
    (65536, 8, 4, 4, 1),               # 65536 walked frames: the grid's z
    (1, 65535 * 32 + 1, 4, 4, 1),      # the grid's y
    (30, 200, 316, 14400, 1),          # 128-row tiles (enough workgroups for them): 316 x 129 x 4 + 1024 bytes of LDS > 160 KB
    (1, 8, 1240, 4, 1),                # 32-row tiles: 1240 x 33 x 4 + 256 bytes > 160 KB
])
def test_beyond_its_bounds_the_entry_answers_not_implemented_before_any_launch(host, sizes):
    lib = _lib.load()
    assert _call(lib, host, *sizes) == _lib.ERR_NOT_IMPLEMENTED, sizes
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_wrapper_refuses_cpu_tensors_with_the_standard_sentence():
    me, feats = torch.zeros(2, 3, 4), torch.zeros(2, 4, 2, 2)
    with pytest.raises(RuntimeError) as e:
        semantic_ops.semantic_quality_counts(me, feats, 1)
    assert str(e.value) == str(ops._cpu_refusal("semantic_quality_counts", "tensor on cpu"))
    assert "Not implemented on the CPU" in str(e.value)
    assert not hasattr(ops, "semantic_quality_counts")              # (ops.py's public set is pinned: the wrapper lives beside it)
