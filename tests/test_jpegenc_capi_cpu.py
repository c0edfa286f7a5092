"""CPU: the fourteenth header of the C ABI (include/univs_jpegenc_hip.h): its symbol is exported and bound, the binding read from it is the
recorded one (tests/jpegenc_capi_signatures.txt), the other tables keep their sizes, its entry answers invalid and uncovered arguments
before any launch, and the wrappers refuse a CPU device with the standard sentence."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, jpegenc_ops, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_jpeg_encode"
COVERED = ("not covered (1 <= W, H <= 16384, (h, v) in {(1, 1), (2, 1), (2, 2)}, 1 <= quality <= 100, 3 N H W < 2^31, raw_total < 2^40, "
           "blocks 16-byte and raw 4-byte aligned)")
ALWAYS = ("rgb", "blocks", "sizes", "bit_off", "totals", "status")
STREAM = ("raw_off", "raw", "out", "out_len")


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_jpegenc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert _declared() == [NAME] == sorted(_lib.JPEGENC_SIGNATURES)
    lib = _lib.load()
    assert hasattr(raw, NAME), f"{NAME} declared in include/univs_jpegenc_hip.h but not exported"
    res, args = _lib.JPEGENC_SIGNATURES[NAME]
    assert getattr(lib, NAME).restype is res and list(getattr(lib, NAME).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "jpegenc_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.JPEGENC_SIGNATURES) == recorded == [NAME + " I PPIPIIIIIIIIIPPPPPLPPPPP"]
    others = (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES) |
              set(_lib.SEMANTIC_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.SWIN_SIGNATURES) | set(_lib.FRAMES_SIGNATURES) |
              set(_lib.PROMPTS_SIGNATURES) | set(_lib.PNG_SIGNATURES) | set(_lib.HOTA_SIGNATURES) | set(_lib.PNGREAD_SIGNATURES) |
              set(_lib.JPEG_SIGNATURES))
    assert not set(_lib.JPEGENC_SIGNATURES) & others
    assert (len(_lib.SIGNATURES), len(_lib.PNG_SIGNATURES), len(_lib.HOTA_SIGNATURES), len(_lib.PNGREAD_SIGNATURES), len(_lib.JPEG_SIGNATURES)) == \
        (76, 1, 2, 1, 1)
    assert "jpeg_encode.hip" in build.SOURCES and any(h.endswith("univs_jpegenc_hip.h") for h in build.HEADERS)
    assert any(h.endswith("jpeg_huff_std.h") for h in build.HEADERS)


def _call(lib, p, ids=None, ids_is_i32=0, lut=None, K=0, edge=-1, N=1, H=48, W=64, h=2, v=2, quality=90, phases=3, raw_total=64, null=(),
          blocks=None, raw=None):
    a = {k: (None if k in null else p) for k in ALWAYS + STREAM}
    a["blocks"] = a["blocks"] if blocks is None else blocks
    a["raw"] = a["raw"] if raw is None else raw
    return getattr(lib, NAME)(a["rgb"], ids, ids_is_i32, lut, K, edge, N, H, W, h, v, quality, phases, a["blocks"], a["sizes"], a["bit_off"],
                              a["totals"], a["raw_off"], raw_total, a["raw"], a["out"], a["out_len"], a["status"], None)


@pytest.fixture
def host():
    """A host buffer's address (16-byte aligned): never read, the entry answers before any launch."""
    buf = (ctypes.c_longlong * 66)()
    yield (ctypes.addressof(buf) + 15) & ~15
    del buf


@pytest.mark.parametrize("kw", [dict(N=-1), dict(phases=0), dict(phases=4), dict(raw_total=-1), dict(ids=1, lut=1, K=0), dict(ids=1, lut=1, K=3, edge=-2),
                                dict(ids=1, lut=1, K=3, edge=1 << 24)])
def test_bad_sizes_are_invalid_arguments(host, kw):
    lib = _lib.load()
    kw = {k: (host if k in ("ids", "lut") else x) for k, x in kw.items()}
    assert _call(lib, host, **kw) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode().startswith(NAME + ": bad arguments N=")


@pytest.mark.parametrize("null", ALWAYS + STREAM)
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


def test_ids_need_a_table_and_phase_1_needs_no_stream_buffers(host):
    lib = _lib.load()
    assert _call(lib, host, ids=host, K=3) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"
    # phases == 1 with the stream pointers NULL passes the pointer check: the next answer is the coverage's
    assert _call(lib, host, phases=1, null=STREAM, quality=0) == _lib.ERR_NOT_IMPLEMENTED


@pytest.mark.parametrize("kw", [dict(W=0), dict(H=0), dict(W=16385), dict(H=16385), dict(h=1, v=2), dict(h=4, v=1), dict(h=2, v=4), dict(quality=0),
                                dict(quality=101), dict(N=60, W=4096, H=4096), dict(raw_total=1 << 40)])
def test_beyond_its_coverage_the_entry_answers_not_implemented_before_any_launch(host, kw):
    lib = _lib.load()
    assert _call(lib, host, **kw) == _lib.ERR_NOT_IMPLEMENTED
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_misaligned_buffers_are_not_covered(host):
    lib = _lib.load()
    assert _call(lib, host, blocks=host + 8) == _lib.ERR_NOT_IMPLEMENTED
    assert _call(lib, host, raw=host + 2) == _lib.ERR_NOT_IMPLEMENTED


def test_no_frames_is_success_without_a_launch():
    assert _call(_lib.load(), None, N=0) == _lib.OK                 # (NULL pointers: nothing is read)


def test_wrappers_refuse_a_cpu_device_with_the_standard_sentence():
    rgb = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    for fn in (lambda: jpegenc_ops.encode_jpegs(rgb), lambda: jpegenc_ops.encode_covered(rgb)):
        with pytest.raises(RuntimeError) as e:
            fn()
        assert str(e.value) == str(ops._cpu_refusal("encode_jpegs", "tensor on cpu"))
    from univs_amd.inference.results import write_overlay_jpegs
    assert not hasattr(ops, "encode_jpegs")                          # (ops.py's public set is pinned: the wrapper lives beside it)
    assert jpegenc_ops.status_text(0) == "ok" and jpegenc_ops.status_text(5) == "DC category above 11, stream region too small"
    assert callable(write_overlay_jpegs)
