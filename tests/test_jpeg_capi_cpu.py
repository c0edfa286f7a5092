"""CPU: the thirteenth header of the C ABI (include/univs_jpeg_hip.h): its symbol is exported and bound, the binding read from it is the
recorded one (tests/jpeg_capi_signatures.txt), its entry answers invalid and uncovered arguments before any launch, and the wrappers
refuse a CPU device with the standard sentence."""
import ctypes
import os
import re

import pytest

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, jpeg_ops, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_jpeg_decode"
COVERED = ("not covered (16 <= W, H <= 16384, (ncomp, h, v) in {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}, subseq_bits a multiple of 32 in "
           "[32, 2^20], max_intervals <= 2^20, src_total and 3 N H W < 2^31, out 4-byte and planes 8-byte aligned)")
POINTERS = ("src", "src_off", "ri", "huff", "quant", "comp", "ivl", "blocks", "planes", "out", "status", "rounds")


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_jpeg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert _declared() == [NAME] == sorted(_lib.JPEG_SIGNATURES)
    lib = _lib.load()
    assert hasattr(raw, NAME), f"{NAME} declared in include/univs_jpeg_hip.h but not exported"
    res, args = _lib.JPEG_SIGNATURES[NAME]
    assert getattr(lib, NAME).restype is res and list(getattr(lib, NAME).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "jpeg_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.JPEG_SIGNATURES) == recorded == [NAME + " I PPPPPIIIIIIIILIPPPPPPPP"]
    others = (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES) |
              set(_lib.SEMANTIC_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.SWIN_SIGNATURES) | set(_lib.FRAMES_SIGNATURES) |
              set(_lib.PROMPTS_SIGNATURES) | set(_lib.PNG_SIGNATURES) | set(_lib.HOTA_SIGNATURES) | set(_lib.PNGREAD_SIGNATURES))
    assert not set(_lib.JPEG_SIGNATURES) & others
    assert (len(_lib.SIGNATURES), len(_lib.PNG_SIGNATURES), len(_lib.HOTA_SIGNATURES), len(_lib.PNGREAD_SIGNATURES)) == (76, 1, 2, 1)
    assert "jpeg_decode.hip" in build.SOURCES and any(h.endswith("univs_jpeg_hip.h") for h in build.HEADERS)
    assert any(h.endswith("jpeg_entropy_core.h") for h in build.HEADERS)


def _call(lib, p, N=1, W=64, H=48, ncomp=3, h=2, v=2, subseq_bits=1024, max_intervals=1, src_total=100, phases=3, null=(), out=None, planes=None):
    a = {k: (None if k in null else p) for k in POINTERS}
    a["out"] = a["out"] if out is None else out
    a["planes"] = a["planes"] if planes is None else planes
    return getattr(lib, NAME)(a["src"], a["src_off"], a["ri"], a["huff"], a["quant"], N, W, H, ncomp, h, v, subseq_bits, max_intervals, src_total,
                              phases, a["comp"], a["ivl"], a["blocks"], a["planes"], a["out"], a["status"], a["rounds"], None)


@pytest.fixture
def host():
    """A host buffer's address (8-byte aligned): never read, the entry answers before any launch."""
    buf = (ctypes.c_longlong * 64)()
    yield ctypes.addressof(buf)
    del buf


@pytest.mark.parametrize("kw", [dict(N=-1), dict(src_total=-1), dict(max_intervals=0), dict(phases=0), dict(phases=4)])
def test_bad_sizes_are_invalid_arguments(host, kw):
    lib = _lib.load()
    assert _call(lib, host, **kw) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode().startswith(NAME + ": bad arguments N=")


@pytest.mark.parametrize("null", POINTERS)
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


@pytest.mark.parametrize("kw", [dict(W=15), dict(H=15), dict(W=16385), dict(H=16385), dict(ncomp=2), dict(ncomp=4), dict(h=1, v=2), dict(h=4, v=1),
                                dict(ncomp=1), dict(subseq_bits=0), dict(subseq_bits=48), dict(subseq_bits=2 ** 20 + 32), dict(max_intervals=2 ** 20 + 1),
                                dict(src_total=2 ** 31), dict(N=60, W=4096, H=4096)])
def test_beyond_its_coverage_the_entry_answers_not_implemented_before_any_launch(host, kw):
    lib = _lib.load()
    assert _call(lib, host, **kw) == _lib.ERR_NOT_IMPLEMENTED
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_misaligned_buffers_are_not_covered(host):
    lib = _lib.load()
    assert _call(lib, host, out=host + 2) == _lib.ERR_NOT_IMPLEMENTED
    assert _call(lib, host, planes=host + 4) == _lib.ERR_NOT_IMPLEMENTED


def test_no_files_is_success_without_a_launch():
    assert _call(_lib.load(), None, N=0) == _lib.OK                 # (NULL pointers: nothing is read)


def test_wrappers_refuse_a_cpu_device_with_the_standard_sentence():
    for fn in (lambda: jpeg_ops.decode_jpegs([b"x"], "cpu"), lambda: jpeg_ops.decode_covered([], "cpu"),
               lambda: jpeg_ops.decode_runs([b"x"], "cpu", None)):
        with pytest.raises(RuntimeError) as e:
            fn()
        assert str(e.value) == str(ops._cpu_refusal("decode_jpegs", "device cpu"))
    with pytest.raises(ValueError, match="subseq_bits"):
        jpeg_ops.decode_jpegs([b"x"], "cuda", subseq_bits=48)
    assert not hasattr(ops, "decode_jpegs")                          # (ops.py's public set is pinned: the wrapper lives beside it)
