"""CPU: the fourth header of the C ABI (include/univs_pvos_hip.h): its symbol is exported and bound, the binding read from it is the
recorded one (tests/pvos_capi_signatures.txt), it shares no symbol with the three other tables, and its entry answers invalid and
uncovered arguments before any launch."""
import ctypes
import os
import re

import pytest

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build
from univs_amd.evaluation import pvos_counts as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_pvos_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == ["univs_pvos_counts"] == sorted(_lib.PVOS_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_pvos_hip.h but not exported"
        res, args = _lib.PVOS_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "pvos_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.PVOS_SIGNATURES) == recorded == ["univs_pvos_counts I PPIIIIIPP"]
    others = set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES) | set(_lib.FUSED_SIGNATURES)
    assert not set(_lib.PVOS_SIGNATURES) & others
    assert len(_lib.SIGNATURES) == 76 and len(_lib.EVAL_SIGNATURES) == 1 and len(_lib.FUSED_SIGNATURES) == 3


def _call(lib, p, T, H, W, d, K, gt=True, pred=True, counts=True):
    return lib.univs_pvos_counts(p if gt else None, p if pred else None, T, H, W, d, K, p if counts else None, None)


@pytest.fixture
def host():
    """A host buffer's address: never read, the entry answers before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


@pytest.mark.parametrize("sizes", [(0, 4, 4, 1, 1), (1, 0, 4, 1, 1), (1, 4, -1, 1, 1), (1, 4, 4, 0, 1), (1, 4, 4, 1, 0), (1, 4, 4, -3, 256)])
def test_bad_sizes_are_invalid_arguments(host, sizes):
    lib = _lib.load()
    assert _call(lib, host, *sizes) == _lib.ERR_INVALID_ARGUMENT
    msg = lib.univs_last_error().decode()
    assert msg == "univs_pvos_counts: bad arguments T=%d H=%d W=%d d=%d K=%d" % sizes


@pytest.mark.parametrize("null", ["gt", "pred", "counts"])
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, 1, 4, 4, 1, 1, **{null: False}) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == "univs_pvos_counts: NULL data pointer"


def test_beyond_its_bounds_the_entry_answers_not_implemented_before_any_launch(host):
    lib = _lib.load()
    for sizes in ((1, 4, 4, pc.D_MAX + 1, 1), (1, 4, 4, 1, pc.K_MAX + 1), (2, 32768, 32768, 1, 1), (1, 65536, 32768, 1, 1)):
        assert _call(lib, host, *sizes) == _lib.ERR_NOT_IMPLEMENTED, sizes
        assert lib.univs_last_error().decode() == f"univs_pvos_counts: not covered (d <= {pc.D_MAX}, K <= {pc.K_MAX}, T H W < 2^31)"
    assert pc.D_MAX >= 44                                             # a 1080 x 1920 frame is covered
