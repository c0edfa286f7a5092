"""CPU: the fifteenth header of the C ABI (include/univs_idmap_hip.h): its two symbols are exported and bound, the binding read from it is
the recorded one (tests/idmap_capi_signatures.txt), it shares no symbol with the fourteen other tables, its entries answer invalid and
uncovered arguments before any launch, and the wrappers refuse CPU tensors with the standard sentence."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, idmap_ops, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS, PROMPTS = "univs_idmap_census_u8", "univs_idmap_prompts_u8"
CENSUS_POINTERS = ("ids", "count", "box")
PROMPTS_POINTERS = ("ids", "frame", "value", "ty", "tx", "masks", "boxes")


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_idmap_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == [CENSUS, PROMPTS] == sorted(_lib.IDMAP_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_idmap_hip.h but not exported"
        res, args = _lib.IDMAP_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signatures_are_the_recorded_ones_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "idmap_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.IDMAP_SIGNATURES) == recorded == [CENSUS + " I PIIIPPP", PROMPTS + " I PIIIPPIPPIIPPP"]
    others = (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES) |
              set(_lib.SEMANTIC_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.SWIN_SIGNATURES) | set(_lib.FRAMES_SIGNATURES) |
              set(_lib.PROMPTS_SIGNATURES) | set(_lib.PNG_SIGNATURES) | set(_lib.HOTA_SIGNATURES) | set(_lib.PNGREAD_SIGNATURES) |
              set(_lib.JPEG_SIGNATURES) | set(_lib.JPEGENC_SIGNATURES))
    assert not set(_lib.IDMAP_SIGNATURES) & others
    assert (len(_lib.SIGNATURES), len(_lib.PROMPTS_SIGNATURES), len(_lib.PNGREAD_SIGNATURES), len(_lib.JPEGENC_SIGNATURES)) == (76, 1, 1, 1)
    assert "idmap_prompts.hip" in build.SOURCES and any(h.endswith("univs_idmap_hip.h") for h in build.HEADERS)


def _census(lib, p, F, H, W, null=()):
    a = {k: (None if k in null else p) for k in CENSUS_POINTERS}
    return getattr(lib, CENSUS)(a["ids"], F, H, W, a["count"], a["box"], None)


def _prompts(lib, p, F, H, W, N, Ho, Wo, null=()):
    a = {k: (None if k in null else p) for k in PROMPTS_POINTERS}
    return getattr(lib, PROMPTS)(a["ids"], F, H, W, a["frame"], a["value"], N, a["ty"], a["tx"], Ho, Wo, a["masks"], a["boxes"], None)


@pytest.fixture
def host():
    """A host buffer's address: never read, the entries answer before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


@pytest.mark.parametrize("sizes", [(-1, 4, 4), (1, 0, 4), (1, 4, -2), (0, 0, 4)])
def test_census_bad_sizes_are_invalid_arguments(host, sizes):
    lib = _lib.load()
    assert _census(lib, host, *sizes) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == CENSUS + ": bad arguments F=%d H=%d W=%d" % sizes


@pytest.mark.parametrize("sizes", [(-1, 4, 4, 1, 4, 4), (1, 0, 4, 1, 4, 4), (1, 4, -3, 1, 4, 4), (1, 4, 4, -1, 4, 4), (1, 4, 4, 1, 0, 4),
                                   (1, 4, 4, 1, 4, 0), (0, 4, 4, 1, 4, 4), (1, 4, 4, 0, -2, 4)])
def test_prompts_bad_sizes_are_invalid_arguments(host, sizes):
    lib = _lib.load()
    assert _prompts(lib, host, *sizes) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == PROMPTS + ": bad arguments F=%d H=%d W=%d N=%d Ho=%d Wo=%d" % sizes


@pytest.mark.parametrize("null", CENSUS_POINTERS)
def test_census_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _census(lib, host, 1, 4, 4, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == CENSUS + ": NULL data pointer"


@pytest.mark.parametrize("null", PROMPTS_POINTERS)
def test_prompts_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _prompts(lib, host, 1, 4, 4, 1, 4, 4, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == PROMPTS + ": NULL data pointer"


@pytest.mark.parametrize("sizes", [(1, 50000, 50000),                # 2.5e9 source pixels
                                   (40000, 300, 200)])               # ... as many small frames
def test_beyond_its_bound_the_census_answers_not_implemented_before_any_launch(host, sizes):
    lib = _lib.load()
    assert _census(lib, host, *sizes) == _lib.ERR_NOT_IMPLEMENTED, sizes
    assert lib.univs_last_error().decode() == f"{CENSUS}: not covered (F H W < 2^31)"


@pytest.mark.parametrize("sizes", [
    (1, 50000, 50000, 1, 8, 8),          # 2.5e9 source pixels
    (40000, 300, 200, 1, 8, 8),          # ... as many small frames
    (1, 100, 100, 1, 50000, 50000),      # 2.5e9 result bytes
    (1, 100, 100, 40000, 300, 200),      # ... as many small planes
])
def test_beyond_each_of_its_two_bounds_the_prompts_answer_not_implemented_before_any_launch(host, sizes):
    lib = _lib.load()
    assert _prompts(lib, host, *sizes) == _lib.ERR_NOT_IMPLEMENTED, sizes
    assert lib.univs_last_error().decode() == f"{PROMPTS}: not covered (F H W < 2^31, N Ho Wo < 2^31)"


def test_no_frames_and_no_objects_are_success_without_a_launch():
    lib = _lib.load()
    assert _census(lib, None, 0, 4, 4) == _lib.OK                    # (NULL pointers: nothing is read)
    assert _prompts(lib, None, 1, 4, 4, 0, 4, 4) == _lib.OK
    assert _prompts(lib, None, 0, 4, 4, 0, 4, 4) == _lib.OK


def test_wrappers_refuse_cpu_tensors_with_the_standard_sentence():
    ids = torch.zeros((1, 4, 4), dtype=torch.uint8)
    lists = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError) as e:
        idmap_ops.idmap_census_u8(ids)
    assert str(e.value) == str(ops._cpu_refusal("idmap_census_u8", "tensor on cpu"))
    with pytest.raises(RuntimeError) as e:
        idmap_ops.idmap_prompts_u8(ids, lists, lists, (2, 2))
    assert str(e.value) == str(ops._cpu_refusal("idmap_prompts_u8", "tensor on cpu"))
    assert "Not implemented on the CPU" in str(e.value)
    assert not hasattr(ops, "idmap_census_u8") and not hasattr(ops, "idmap_prompts_u8")   # (ops.py's public set is pinned)
