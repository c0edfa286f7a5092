"""CPU: the twelfth header of the C ABI (include/univs_pngread_hip.h): its symbol is exported and bound, the binding read from it is the
recorded one (tests/pngread_capi_signatures.txt), its entry answers invalid and uncovered arguments before any launch, and the wrapper
refuses a CPU device with the standard sentence."""
import ctypes
import os
import re

import pytest

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, ops, png_read_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_png_read"
COVERED = "not covered (max_rowbytes <= 24576, streams_total, filt_total and out_total < 2^31)"
POINTERS = ("streams", "stream_offsets", "desc", "filt_offsets", "out_offsets", "filtered", "out", "status")


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_pngread_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert _declared() == [NAME] == sorted(_lib.PNGREAD_SIGNATURES)
    lib = _lib.load()
    assert hasattr(raw, NAME), f"{NAME} declared in include/univs_pngread_hip.h but not exported"
    res, args = _lib.PNGREAD_SIGNATURES[NAME]
    assert getattr(lib, NAME).restype is res and list(getattr(lib, NAME).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "pngread_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.PNGREAD_SIGNATURES) == recorded == [NAME + " I PPPPIPPILLLIPPPP"]
    others = (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES) |
              set(_lib.SEMANTIC_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.SWIN_SIGNATURES) | set(_lib.FRAMES_SIGNATURES) |
              set(_lib.PROMPTS_SIGNATURES) | set(_lib.PNG_SIGNATURES) | set(_lib.HOTA_SIGNATURES))
    assert not set(_lib.PNGREAD_SIGNATURES) & others
    assert (len(_lib.SIGNATURES), len(_lib.PNG_SIGNATURES), len(_lib.HOTA_SIGNATURES)) == (76, 1, 2)
    assert "png_inflate.hip" in build.SOURCES and any(h.endswith("univs_pngread_hip.h") for h in build.HEADERS)
    assert any(h.endswith("png_inflate_core.h") for h in build.HEADERS)


def _call(lib, p, N=1, P=0, palettes=False, totals=(10, 10, 10), max_rowbytes=8, null=()):
    a = {k: (None if k in null else p) for k in POINTERS}
    return getattr(lib, NAME)(a["streams"], a["stream_offsets"], a["desc"], p if palettes else None, P, a["filt_offsets"], a["out_offsets"], N,
                              *totals, max_rowbytes, a["filtered"], a["out"], a["status"], None)


@pytest.fixture
def host():
    """A host buffer's address: never read, the entry answers before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


@pytest.mark.parametrize("kw", [dict(N=-1), dict(P=-1), dict(P=2), dict(totals=(-1, 10, 10)), dict(totals=(10, -1, 10)),
                                dict(totals=(10, 10, -1)), dict(max_rowbytes=0)])
def test_bad_sizes_are_invalid_arguments(host, kw):
    lib = _lib.load()
    assert _call(lib, host, **kw) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode().startswith(NAME + ": bad arguments N=")


@pytest.mark.parametrize("null", POINTERS)
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


@pytest.mark.parametrize("kw", [dict(max_rowbytes=24577), dict(totals=(2 ** 31, 10, 10)), dict(totals=(10, 2 ** 31, 10)),
                                dict(totals=(10, 10, 2 ** 31))])
def test_beyond_its_bounds_the_entry_answers_not_implemented_before_any_launch(host, kw):
    lib = _lib.load()
    assert _call(lib, host, **kw) == _lib.ERR_NOT_IMPLEMENTED
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_no_files_is_success_without_a_launch():
    assert _call(_lib.load(), None, N=0) == _lib.OK                 # (NULL pointers: nothing is read)


def test_wrapper_refuses_a_cpu_device_with_the_standard_sentence():
    with pytest.raises(RuntimeError) as e:
        png_read_ops.read_pngs_device([b"x"], "cpu")
    assert str(e.value) == str(ops._cpu_refusal("read_pngs_device", "device cpu"))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        png_read_ops.read_covered([], "cpu")
    with pytest.raises(ValueError):
        png_read_ops.read_pngs_device([b"x"], "cuda", uncovered="pillow")
    assert not hasattr(ops, "read_pngs_device")                     # (ops.py's public set is pinned: the wrapper lives beside it)
