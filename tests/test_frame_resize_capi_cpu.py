"""CPU: the eighth header of the C ABI (include/univs_frames_hip.h): its symbol is exported and bound, the binding read from it is the
recorded one (tests/frames_capi_signatures.txt), it shares no symbol with the seven other tables, its entry answers invalid and uncovered
arguments before any launch, and the wrapper refuses CPU tensors with the standard sentence."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, frames_ops, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_resize_frames_u8"
COVERED = "not covered (ksize_x <= 9 and ksize_y <= 9: a down-scale up to 4; T Hi Wi 3 < 2^31, T 3 Ho Wo < 2^31)"


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_frames_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == [NAME] == sorted(_lib.FRAMES_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_frames_hip.h but not exported"
        res, args = _lib.FRAMES_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "frames_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.FRAMES_SIGNATURES) == recorded == [NAME + " I PIIIIIPPPIPPPIIPP"]
    others = (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES) |
              set(_lib.SEMANTIC_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.SWIN_SIGNATURES))
    assert not set(_lib.FRAMES_SIGNATURES) & others
    assert "frame_resize.hip" in build.SOURCES and any(h.endswith("univs_frames_hip.h") for h in build.HEADERS)


def ksize(n_in, n_out):
    return 2 * -(-max(n_in, n_out) // n_out) + 1


def _call(lib, p, T, Hi, Wi, Ho, Wo, ksx=None, ksy=None, null=()):
    a = {k: (None if k in null else p) for k in ("src", "first_x", "count_x", "coef_x", "first_y", "count_y", "coef_y", "out")}
    return getattr(lib, NAME)(a["src"], T, Hi, Wi, Ho, Wo, a["first_x"], a["count_x"], a["coef_x"], ksize(Wi, Wo) if ksx is None else ksx,
                              a["first_y"], a["count_y"], a["coef_y"], ksize(Hi, Ho) if ksy is None else ksy, 0, a["out"], None)


@pytest.fixture
def host():
    """A host buffer's address: never read, the entry answers before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


@pytest.mark.parametrize("sizes", [(0, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, -1, 4, 4), (1, 4, 4, 0, 4), (1, 4, 4, 4, 0), (-2, 4, 4, -7, 4)])
def test_bad_sizes_are_invalid_arguments(host, sizes):
    lib = _lib.load()
    assert _call(lib, host, *sizes, ksx=3, ksy=3) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": bad arguments T=%d Hi=%d Wi=%d Ho=%d Wo=%d" % sizes


@pytest.mark.parametrize("ks", [(3, 5), (5, 3), (7, 5), (5, 0)])
def test_a_ksize_that_is_not_the_axis_own_is_an_invalid_argument(host, ks):
    lib = _lib.load()
    assert _call(lib, host, 1, 37, 53, 20, 29, ksx=ks[0], ksy=ks[1]) == _lib.ERR_INVALID_ARGUMENT       # both axes have 5 slots
    assert lib.univs_last_error().decode() == (f"{NAME}: ksize_x={ks[0]} ksize_y={ks[1]}, but 53 -> 29 columns have 5 slots and "
                                               "37 -> 20 rows 5")


@pytest.mark.parametrize("sizes,null", [((1, 37, 53, 20, 29), "src"), ((1, 37, 53, 20, 29), "out"), ((1, 37, 53, 20, 29), "coef_x"),
                                        ((1, 37, 53, 20, 29), "first_y"), ((1, 37, 53, 37, 29), "count_x"), ((1, 37, 53, 20, 53), "coef_y")])
def test_null_pointers_are_invalid_arguments(host, sizes, null):
    lib = _lib.load()
    assert _call(lib, host, *sizes, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


@pytest.mark.parametrize("sizes", [
    (1, 64, 96, 5, 7),                 # a down-scale by 12.8: 27 slots
    (1, 48, 64, 1, 1),                 # everything into one pixel
    (1, 96, 129, 24, 32),              # just beyond 4 on one axis: 11 slots
    (2, 20000, 20000, 20000, 10000),   # 2.4e9 source bytes
    (1, 100, 100, 30000, 30000),       # 2.7e9 result bytes
])
def test_beyond_its_bounds_the_entry_answers_not_implemented_before_any_launch(host, sizes):
    lib = _lib.load()
    assert _call(lib, host, *sizes) == _lib.ERR_NOT_IMPLEMENTED, sizes
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_wrapper_refuses_cpu_tensors_with_the_standard_sentence():
    frames = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError) as e:
        frames_ops.resize_frames_u8(frames, (4, 4))
    assert str(e.value) == str(ops._cpu_refusal("resize_frames_u8", "tensor on cpu"))
    assert "Not implemented on the CPU" in str(e.value)
    assert not hasattr(ops, "resize_frames_u8")                     # (ops.py's public set is pinned: the wrapper lives beside it)
