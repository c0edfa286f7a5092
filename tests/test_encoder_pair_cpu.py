"""CPU: the sixth header of the C ABI (include/univs_encoder_hip.h) and the plan of its kernel (csrc/linear_pair_f16x3.hip):
  * its symbol is exported and bound, the binding read from it is the recorded one (tests/encoder_capi_signatures.txt), it shares no
    symbol with the five other tables and they keep theirs;
  * the entry answers invalid and uncovered arguments before any launch (host pointers that are never read);
  * the plan (tools/encoder_pair_plan.cpp over csrc/gemm_plan.h, hipcc's host compiler) covers every (row tile, feature group) of both
    problems exactly once at 64, 256 and 304 CUs, for the model's shape and the GPU file's;
  * the wrapper refuses CPU tensors with the standard sentence, and the switch defaults on."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, encoder_ops, ops
from univs_amd.switches import Switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_encoder_linear_pair_presplit_f32"
COVERED = ("not covered (K == 256, add_rows == rows_per_batch dividing M, N_a in passes of 113 .. 128 features and N_b of 81 .. 96, "
           "column blocks of a multiple of 4 dividing N, 16-byte aligned pointers, M max(K, N_a, N_b) 4 < 2^31)")
# the model's clip (T = 5 frames of 19 320 tokens), then the shapes of tests/test_encoder_pair_gpu.py: (T, S) -> M = T S, with B of 288 / 96
PLAN_CASES = [(96600, 256, 288), (40, 256, 288), (903, 256, 288), (8226, 256, 288), (903, 256, 96)]


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_encoder_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == [NAME] == sorted(_lib.ENCODER_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_encoder_hip.h but not exported"
        res, args = _lib.ENCODER_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "encoder_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.ENCODER_SIGNATURES) == recorded == [NAME + " I PPLPPPIIPPPPIIPLILP"]
    tables = (_lib.SIGNATURES, _lib.EVAL_SIGNATURES, _lib.FUSED_SIGNATURES, _lib.PVOS_SIGNATURES, _lib.SEMANTIC_SIGNATURES)
    assert not set(_lib.ENCODER_SIGNATURES) & set().union(*tables)
    assert tuple(len(t) for t in tables) == (76, 1, 3, 1, 1)
    assert "linear_pair_f16x3.hip" in build.SOURCES and any(h.endswith("univs_encoder_hip.h") for h in build.HEADERS)


@pytest.fixture
def host():
    """A 16-byte aligned host address: never read, the entry answers before any launch."""
    buf = (ctypes.c_char * 256)()
    yield (ctypes.addressof(buf) + 15) // 16 * 16
    del buf


def _call(lib, p, M=8226, K=256, add_rows=4113, rows=4113, Na=256, ca=32, Nb=288, cb=36, null=(), off=None):
    """All pointers `p` (the one named `off` 4 bytes further, those in `null` NULL; the biases may be NULL)"""
    a = {k: (None if k in null else p + (4 if k == off else 0)) for k in ("x", "add", "wpa", "wia", "ba", "ya", "wpb", "wib", "bb", "yb")}
    return getattr(lib, NAME)(a["x"], a["add"], add_rows, a["wpa"], a["wia"], a["ba"], Na, ca, a["ya"], a["wpb"], a["wib"], a["bb"], Nb, cb,
                              a["yb"], M, K, rows, None)


@pytest.mark.parametrize("bad", [dict(M=0), dict(M=-4113), dict(K=0), dict(add_rows=0), dict(rows=-1), dict(Na=0), dict(Nb=-288), dict(ca=0),
                                 dict(cb=0)])
def test_bad_sizes_are_invalid_arguments(host, bad):
    lib = _lib.load()
    assert _call(lib, host, **bad) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode().startswith(NAME + ": bad arguments M=")


@pytest.mark.parametrize("null", ["x", "add", "wpa", "wia", "ya", "wpb", "wib", "yb"])
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


@pytest.mark.parametrize("case", [
    dict(M=8226 + 1),                                   # M % add_rows != 0
    dict(M=8226, add_rows=2742, rows=4113),             # add_rows != rows_per_batch (both divide M)
    dict(K=128), dict(K=192), dict(K=512), dict(K=1024),   # K outside the blocked resident kernel's
    dict(Na=240), dict(Nb=280),                         # N not a multiple of the block width
    dict(ca=34, Na=272), dict(cb=6),                    # a block width that is no multiple of 4
    dict(Na=192, ca=32), dict(Nb=256, cb=32), dict(Nb=64, cb=32),   # passes that are not the built kernel's (A: 2 x 96; B: 2 x 128, 1 x 64)
    dict(off="x"), dict(off="add"), dict(off="wpa"), dict(off="wia"), dict(off="ba"), dict(off="ya"), dict(off="wpb"), dict(off="wib"),
    dict(off="bb"), dict(off="yb"),                     # misaligned pointers
    dict(M=1863680 * 2, add_rows=1863680, rows=1863680),   # M N_b 4 >= 2^31: byte offsets beyond a buffer descriptor's range
    dict(M=2 ** 21, add_rows=2 ** 20, rows=2 ** 20),    # M K 4 = 2^31
])
def test_what_the_entry_does_not_cover_is_not_implemented_before_any_launch(host, case):
    lib = _lib.load()
    assert _call(lib, host, **case) == _lib.ERR_NOT_IMPLEMENTED, case
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_null_biases_are_accepted_by_the_checks(host):
    """(up to the launch: the uncovered K answers after the NULL check, so a NULL bias is no NULL data pointer)"""
    lib = _lib.load()
    assert _call(lib, host, K=128, null=("ba", "bb")) == _lib.ERR_NOT_IMPLEMENTED


def test_plan_covers_both_problems_exactly_once_at_every_cu_count(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "encoder_pair_plan")
    subprocess.run([hipcc, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "encoder_pair_plan.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    lines = "".join(f"{M} {Na} {Nb} 256\n" for M, Na, Nb in PLAN_CASES)
    run = subprocess.run([exe], input=lines, capture_output=True, text=True, timeout=120)
    out = [l.split() for l in run.stdout.splitlines()]
    assert run.returncode == 0 and len(out) == 3 * len(PLAN_CASES), run.stdout
    for (M, Na, Nb), n_cu, l in zip([c for c in PLAN_CASES for _ in range(3)], [64, 256, 304] * len(PLAN_CASES), out):
        assert l[:5] == [str(M), str(Na), str(Nb), "256", str(n_cu)] and l[5] == "linear_pair_f16x3<8,6,4>" and l[-1] == "once=1", l
        gx, pa, pb, lds = (int(v) for v in l[6:10])
        assert (pa, pb) == (2, -(-Nb // 96)) and gx * (pa + pb) <= n_cu and lds <= 160 * 1024 - 2048
    # the model's clip on the model's card: 51 row ranges x 5 passes, 255 of the 256 CUs
    assert out[1][6:9] == ["51", "2", "3"]


def test_wrapper_refuses_cpu_tensors_and_the_switch_defaults_on():
    x, pos, wa, wb = torch.zeros(2, 8, 256), torch.zeros(1, 8, 256), torch.zeros(256, 256), torch.zeros(288, 256)
    with pytest.raises(RuntimeError) as e:
        encoder_ops.linear_pair_blocked(x, pos, wa, None, 32, wb, None, 36)
    assert str(e.value) == str(ops._cpu_refusal("linear_pair_blocked", "tensor on cpu"))
    assert not hasattr(ops, "linear_pair_blocked")                   # (ops.py's public set is pinned: the wrapper lives beside it)
    assert Switches().encoder_pair is True
