"""CPU: the seventh header of the C ABI (include/univs_swin_hip.h) and the wrapper of its entry (univs_amd/swin_ops.py):
  * its symbol is exported and bound, the binding read from it is the recorded one (tests/swin_capi_signatures.txt), it shares no symbol
    with the six other tables and they keep theirs; the source and the header are in the build's lists;
  * the entry answers invalid and uncovered arguments before any launch (host pointers that are never read);
  * the wrapper refuses CPU tensors with the standard sentence, hands the library's "not covered" on as None, passes the stream last, and
    lives outside ops.py; the switch exists and has an environment name."""
import ctypes
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, ops, swin_ops, switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "univs_swin_window_attention_qkv_presplit_f32"
COVERED = "not covered (7 x 7 windows, C == 32 nH in {96, 192}, x and the weight image 16-byte aligned, B H W C 4 < 2^31 - 1)"


def _declared():
    text = open(os.path.join(ROOT, "include", "univs_swin_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text)))


def test_header_symbol_is_exported_and_bound():
    build.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert names == [NAME] == sorted(_lib.SWIN_SIGNATURES)
    lib = _lib.load()
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/univs_swin_hip.h but not exported"
        res, args = _lib.SWIN_SIGNATURES[n]
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args


def test_signature_is_the_recorded_one_and_the_other_tables_keep_theirs():
    recorded = open(os.path.join(ROOT, "tests", "swin_capi_signatures.txt")).read().splitlines()
    assert signature_lines(_lib.SWIN_SIGNATURES) == recorded == [NAME + " I PPPPPPIIIIIIIFPP"]
    tables = (_lib.SIGNATURES, _lib.EVAL_SIGNATURES, _lib.FUSED_SIGNATURES, _lib.PVOS_SIGNATURES, _lib.SEMANTIC_SIGNATURES, _lib.ENCODER_SIGNATURES)
    assert not set(_lib.SWIN_SIGNATURES) & set().union(*tables)
    assert tuple(len(t) for t in tables) == (76, 1, 3, 1, 1, 1)
    assert "window_attn_qkv.hip" in build.SOURCES and any(h.endswith("univs_swin_hip.h") for h in build.HEADERS)
    assert os.path.exists(os.path.join(build.CSRC, "window_attn_qkv.hip"))


@pytest.fixture
def host():
    """A 16-byte aligned host address: never read, the entry answers before any launch."""
    buf = (ctypes.c_char * 256)()
    yield (ctypes.addressof(buf) + 15) // 16 * 16
    del buf


def _call(lib, p, B=2, H=30, W=45, ws=7, shift=0, nH=3, C=96, null=(), off=None):
    """All pointers `p` (the one named `off` 4 bytes further, those in `null` NULL)"""
    a = {k: (None if k in null else p + (4 if k == off else 0)) for k in ("x", "wp", "winv", "qb", "bias", "mask", "out")}
    return getattr(lib, NAME)(a["x"], a["wp"], a["winv"], a["qb"], a["bias"], a["mask"], B, H, W, ws, shift, nH, C, 32 ** -0.5, a["out"], None)


@pytest.mark.parametrize("bad", [dict(B=-1), dict(H=0), dict(W=0), dict(ws=0), dict(shift=-1), dict(shift=7), dict(nH=0), dict(C=0)])
def test_bad_sizes_are_invalid_arguments(host, bad):
    lib = _lib.load()
    assert _call(lib, host, **bad) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode().startswith(NAME + ": bad dimensions B=")


@pytest.mark.parametrize("null", ["x", "wp", "winv", "bias", "out"])
def test_null_pointers_are_invalid_arguments(host, null):
    lib = _lib.load()
    assert _call(lib, host, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.univs_last_error().decode() == NAME + ": NULL data pointer"


@pytest.mark.parametrize("case", [
    dict(C=128, nH=4), dict(C=384, nH=12), dict(C=64, nH=2),      # widths outside stages 1 and 2
    dict(C=96, nH=6), dict(C=192, nH=3),                         # head_dim != 32
    dict(ws=12), dict(ws=8, shift=3),                            # windows other than 7 x 7
    dict(off="x"), dict(off="wp"),                               # misaligned x / weight image
    dict(B=64, H=736, W=1280, C=96, nH=3),                       # B H W C 4 >= 2^31: byte offsets beyond a buffer descriptor's range
])
def test_what_the_entry_does_not_cover_is_not_implemented_before_any_launch(host, case):
    lib = _lib.load()
    assert _call(lib, host, **case) == _lib.ERR_NOT_IMPLEMENTED, case
    assert lib.univs_last_error().decode() == f"{NAME}: {COVERED}"


def test_empty_batch_and_null_optionals(host):
    """B == 0 is OK before any pointer is looked at; a NULL qkv bias or mask is no NULL data pointer (the uncovered C answers after the
    NULL check)"""
    lib = _lib.load()
    assert _call(lib, host, B=0, null=("x", "out")) == _lib.OK
    assert _call(lib, host, C=128, nH=4, null=("qb", "mask")) == _lib.ERR_NOT_IMPLEMENTED


def test_wrapper_contract(monkeypatch):
    x, w, b, bias = torch.zeros(1, 49, 96), torch.zeros(288, 96), torch.zeros(288), torch.zeros(3, 49, 49)
    with pytest.raises(RuntimeError) as e:
        swin_ops.window_attention_qkv(x, w, b, bias, None, 7, 7, 7, 0, 32 ** -0.5)
    assert str(e.value) == str(ops._cpu_refusal("window_attention_qkv", "tensor on cpu"))
    assert not hasattr(ops, "window_attention_qkv")                  # (ops.py's public set is pinned: the wrapper lives beside it)
    with pytest.raises(RuntimeError):
        swin_ops.window_attention_qkv(x, w[:, :95], b, bias, None, 7, 7, 7, 0, 32 ** -0.5)   # a weight that is not [3C, C]
    # `ops._call` is the launch: the library function first, the anchor tensor, the arguments in the header's order; it appends the stream
    # and its False ("not covered") comes back as None
    seen = {}

    class Lib:
        univs_swin_window_attention_qkv_presplit_f32 = object()

    def fake_call(name, fn, anchor, *args, **kw):
        seen.update(name=name, fn=fn, anchor=anchor, n=len(args), kw=kw)
        return seen["answer"]

    ok = lambda name, *t: None                                       # noqa: E731
    monkeypatch.setattr(ops, "_call", fake_call)
    monkeypatch.setattr(ops, "_require_gpu", ok)
    monkeypatch.setattr(ops, "presplit_weights", lambda w_: (torch.zeros(288 * 96, dtype=torch.int32), torch.zeros(288)))
    monkeypatch.setattr(swin_ops._lib, "load", lambda: Lib)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for answer in (False, True):
        seen["answer"] = answer
        out = swin_ops.window_attention_qkv(x, w, b, bias, None, 7, 7, 7, 0, 32 ** -0.5)
        assert (out is None) == (not answer)
        assert seen["name"] == "window_attention_qkv" and seen["fn"] is Lib.univs_swin_window_attention_qkv_presplit_f32
        assert seen["anchor"].shape == x.shape and seen["kw"] == {}
        assert seen["n"] == len(_lib.SWIN_SIGNATURES[NAME][1]) - 1   # every argument of the header but the stream, which _call appends
    assert out.shape == x.shape


def test_switch_exists_with_its_environment_name():
    assert isinstance(switches.Switches().swin_fused_qkv, bool) and isinstance(switches.SWITCHES.swin_fused_qkv, bool)
    text = open(os.path.join(ROOT, "univs_amd", "switches.py")).read()
    assert 'swin_fused_qkv=_flag("UNIVS_SWIN_FUSED_QKV"' in text
