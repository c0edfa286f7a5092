"""CPU: the seventeenth header of the C ABI (include/univs_imagelabels_hip.h): its two symbols are exported and bound, the binding read
from it is the recorded one (tests/imagelabels_capi_signatures.txt), it shares no symbol with the sixteen other tables, its entries
answer invalid and uncovered arguments before any launch, and the wrappers refuse CPU tensors with the standard sentence."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, imagelabels_ops, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS, CONFUSION = "univs_semseg_labels_f32", "univs_label_confusion_u8"
CONFUSION_POINTERS = ("gt", "pred", "conf", "stray")


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_imagelabels_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_are_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == [CONFUSION, LABELS] == sorted(_lib.IMAGELABELS_BINDING)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_imagelabels_hip.h but not exported"
        res, args = _lib.IMAGELABELS_BINDING[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signatures_are_the_recorded_ones_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "imagelabels_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.IMAGELABELS_BINDING) == recorded == [CONFUSION + " I PPLIIPPP", LABELS + " I PIIIIIPP"]
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES")]
    assert len(others) == 16 and not any(set(_lib.IMAGELABELS_BINDING) & set(t) for t in others)
    assert (len(_lib.SIGNATURES), len(_lib.IDMAP_SIGNATURES), len(_lib.SEAM_SIGNATURES)) == (76, 2, 2)
    assert "semseg_labels.hip" in build.SOURCES and any(h.endswith("univs_imagelabels_hip.h") for h in build.HEADERS)
    assert "semseg_labels.hip" not in build.SOURCE_FLAGS and "resample.hip" not in build.SOURCE_FLAGS   # the same flags: the same roundings


@pytest.fixture
def host():
    """A host buffer's address: never read, the entries answer before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


def _labels(lib, p, C, hi, wi, H, W, null=()):
    return getattr(lib, LABELS)(None if "r" in null else p, C, hi, wi, H, W, None if "labels" in null else p, None)


def _confusion(lib, p, n, K, ignore, null=()):
    a = {k: (None if k in null else p) for k in CONFUSION_POINTERS}
    return getattr(lib, CONFUSION)(a["gt"], a["pred"], n, K, ignore, a["conf"], a["stray"], None)


@pytest.mark.parametrize("sizes", [(0, 4, 4, 4, 4), (3, 0, 4, 4, 4), (3, 4, -1, 4, 4), (3, 4, 4, 0, 4), (3, 4, 4, 4, -5)])
def test_labels_bad_sizes_are_invalid_arguments(host, sizes):
    lib = _lib.load()
    assert _labels(lib, host, *sizes) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == LABELS + ": bad arguments C=%d hi=%d wi=%d H=%d W=%d" % sizes


@pytest.mark.parametrize("args", [(-1, 5, 255), (10, 0, 255), (10, 5, 4), (10, 5, 0), (10, 5, 256), (10, 5, -2)])
def test_confusion_bad_arguments_are_invalid_arguments(host, args):
    lib = _lib.load()
    assert _confusion(lib, host, *args) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == CONFUSION + ": bad arguments n=%d num_classes=%d ignore_label=%d" % args


@pytest.mark.parametrize("null", ("r", "labels"))
def test_labels_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _labels(lib, host, 3, 4, 4, 4, 4, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == LABELS + ": NULL data pointer"


@pytest.mark.parametrize("null", CONFUSION_POINTERS)
def test_confusion_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _confusion(lib, host, 10, 5, 255, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == CONFUSION + ": NULL data pointer"


@pytest.mark.parametrize("sizes", [(257, 4, 4, 4, 4),                # a class is one byte
                                   (3, 4, 4, 50000, 50000),          # 2.5e9 labels
                                   (3, 50000, 50000, 4, 4)])         # 2.5e9 values per plane
def test_beyond_each_of_its_bounds_the_labels_answer_not_implemented_before_any_launch(host, sizes):
    lib = _lib.load()
    assert _labels(lib, host, *sizes) == _lib.ERR_NOT_IMPLEMENTED, sizes
    assert lib.univs_last_error().decode() == f"{LABELS}: not covered (C <= 256, H W < 2^31, hi wi < 2^31)"


@pytest.mark.parametrize("args", [(10, 181, 255),                    # 182^2 = 33124 cells
                                  (2 ** 31 - 4, 5, 255)])            # pixels
def test_beyond_each_of_its_bounds_the_confusion_answers_not_implemented_before_any_launch(host, args):
    lib = _lib.load()
    assert _confusion(lib, host, *args) == _lib.ERR_NOT_IMPLEMENTED, args
    assert lib.univs_last_error().decode() == (f"{CONFUSION}: not covered ((num_classes + 1)^2 <= 32768, n < 2^31 - 4, dword-aligned maps, "
                                               "8-byte aligned counts)")


def test_maps_and_counts_off_their_alignment_are_not_covered(host):
    lib = _lib.load()
    fn = getattr(lib, CONFUSION)
    for off in ((1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 4, 0), (0, 0, 0, 4)):
        assert fn(host + off[0], host + off[1], 10, 5, 255, host + 8 + off[2], host + 16 + off[3], None) == _lib.ERR_NOT_IMPLEMENTED, off


def test_no_pixels_are_success_without_a_launch():
    assert _confusion(_lib.load(), None, 0, 5, 255) == _lib.OK       # (NULL pointers: nothing is read)


def test_wrappers_refuse_cpu_tensors_with_the_standard_sentence():
    with pytest.raises(RuntimeError) as e:
        imagelabels_ops.semseg_labels(torch.zeros((3, 4, 4)), (4, 4))
    assert str(e.value) == str(ops._cpu_refusal("semseg_labels", "tensor on cpu"))
    m = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(RuntimeError) as e:
        imagelabels_ops.label_confusion_u8(m, m, 3, 255, *imagelabels_ops.new_confusion(3, "cpu"))
    assert str(e.value) == str(ops._cpu_refusal("label_confusion_u8", "tensor on cpu"))
    assert "Not implemented on the CPU" in str(e.value)
    assert not hasattr(ops, "semseg_labels") and not hasattr(ops, "label_confusion_u8")   # (ops.py's public set is pinned)
