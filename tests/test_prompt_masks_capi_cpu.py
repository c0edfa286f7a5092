"""CPU: the ninth header of the C ABI (include/univs_prompts_hip.h): its symbol is exported and bound, the binding read from it is the
recorded one (tests/prompts_capi_signatures.txt), it shares no symbol with the eight other tables, its entry answers invalid and
uncovered arguments before any launch, and the wrapper refuses CPU tensors with the standard sentence."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, ops, prompts_ops
from univs_amd.evaluation.vis_counts import Runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_resize_rle_masks_u8"
COVERED = "not covered (H W < 2^31, n_bounds < 2^31, N Ho Wo < 2^31)"
POINTERS = ("bounds", "starts", "ty", "tx", "masks", "boxes")


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_prompts_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == [NAME] == sorted(_lib.PROMPTS_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_prompts_hip.h but not exported"
        res, args = _lib.PROMPTS_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "prompts_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.PROMPTS_SIGNATURES) == recorded == [NAME + " I PPLIIIPPIIPPP"]
    others = (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES) | set(_lib.PVOS_SIGNATURES) |
              set(_lib.SEMANTIC_SIGNATURES) | set(_lib.ENCODER_SIGNATURES) | set(_lib.SWIN_SIGNATURES) | set(_lib.FRAMES_SIGNATURES))
    assert not set(_lib.PROMPTS_SIGNATURES) & others
    assert (len(_lib.SIGNATURES), len(_lib.FRAMES_SIGNATURES)) == (76, 1)
    assert "mask_prompt_resize.hip" in build.SOURCES and any(h.endswith("univs_prompts_hip.h") for h in build.HEADERS)


def _call(lib, p, n_bounds, N, H, W, Ho, Wo, null=()):
    a = {k: (None if k in null else p) for k in POINTERS}
    return getattr(lib, NAME)(a["bounds"], a["starts"], n_bounds, N, H, W, a["ty"], a["tx"], Ho, Wo, a["masks"], a["boxes"], None)


@pytest.fixture
def host():
    """A host buffer's address: never read, the entry answers before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


@pytest.mark.parametrize("sizes", [(4, -1, 4, 4, 4, 4), (-1, 1, 4, 4, 4, 4), (4, 1, 0, 4, 4, 4), (4, 1, 4, -3, 4, 4), (4, 1, 4, 4, 0, 4),
                                   (4, 1, 4, 4, 4, 0), (0, 0, 4, 4, -2, 4)])
def test_bad_sizes_are_invalid_arguments(host, sizes):
    lib = _lib.load()
    assert _call(lib, host, *sizes) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": bad arguments n_bounds=%d N=%d H=%d W=%d Ho=%d Wo=%d" % sizes


@pytest.mark.parametrize("null", POINTERS)
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, 4, 1, 4, 4, 4, 4, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


@pytest.mark.parametrize("sizes", [
    (4, 1, 50000, 50000, 8, 8),          # 2.5e9 source pixels
    (2 ** 31, 1, 100, 100, 8, 8),        # 2^31 boundaries
    (4, 1, 100, 100, 50000, 50000),      # 2.5e9 result bytes
    (4, 40000, 100, 100, 300, 200),      # ... as many small planes
])
def test_beyond_its_bounds_the_entry_answers_not_implemented_before_any_launch(host, sizes):
    lib = _lib.load()
    assert _call(lib, host, *sizes) == _lib.ERR_NOT_IMPLEMENTED, sizes
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_no_masks_is_success_without_a_launch():
    lib = _lib.load()
    assert _call(lib, None, 0, 0, 4, 4, 4, 4) == _lib.OK            # (NULL pointers: nothing is read)


def test_wrapper_refuses_cpu_tensors_with_the_standard_sentence():
    runs = Runs(torch.tensor([3, 16], dtype=torch.int32), torch.tensor([0, 13], dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32))
    with pytest.raises(RuntimeError) as e:
        prompts_ops.resize_rle_masks_u8(runs, (4, 4), (2, 2))
    assert str(e.value) == str(ops._cpu_refusal("resize_rle_masks_u8", "tensor on cpu"))
    assert "Not implemented on the CPU" in str(e.value)
    assert not hasattr(ops, "resize_rle_masks_u8")                  # (ops.py's public set is pinned: the wrapper lives beside it)
