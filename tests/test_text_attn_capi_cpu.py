"""CPU: the eighteenth header of the C ABI (include/univs_text_hip.h): its symbol is exported and bound, it shares no symbol with the other
tables, the entry answers invalid and uncovered arguments before any launch, the wrapper raises on a wrong row table and refuses CPU
tensors with the standard sentence, and the ATen formulation follows the rule on the CPU."""
import ctypes
import math
import os
import re

import pytest
import torch

from tests.test_capi_contract_cpu import signature_lines
from univs_amd import _lib, build, ops, text_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "univs_text_attention_f32"
NOT_COVERED = ENTRY + ": not covered (E / heads in {16, 32, 64}, Lmax <= 128, Ntok 3 E < 2^31, S heads < 2^31)"


def test_header_symbol_is_exported_and_bound():
    build.build()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "univs_text_hip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(univs_[a-z0-9_]+)\s*\(", text))) == [ENTRY] == sorted(_lib.TEXT_BINDING)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), ENTRY)
    res, args = _lib.TEXT_BINDING[ENTRY]
    fn = getattr(_lib.load(), ENTRY)
    assert fn.restype is res and list(fn.argtypes) == args
    assert signature_lines(_lib.TEXT_BINDING) == [ENTRY + " I PPILIIIFPP"]
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES")] + [_lib.IMAGELABELS_BINDING]
    assert not any(set(_lib.TEXT_BINDING) & set(t) for t in others)
    assert "text_attn.hip" in build.SOURCES and any(h.endswith("univs_text_hip.h") for h in build.HEADERS)


@pytest.fixture
def host():
    """A host buffer's address: never read, the entry answers before any launch."""
    buf = (ctypes.c_int * 64)()
    yield ctypes.addressof(buf)
    del buf


def _entry(p, S, Ntok, E, heads, Lmax, null=()):
    a = {k: (None if k in null else p) for k in ("qkv", "start", "out")}
    return getattr(_lib.load(), ENTRY)(a["qkv"], a["start"], S, Ntok, E, heads, Lmax, 0.125, a["out"], None)


@pytest.mark.parametrize("args", [(-1, 4, 64, 4, 8), (1, -4, 64, 4, 8), (1, 4, 0, 4, 8), (1, 4, 64, 0, 8), (1, 4, 64, 3, 8), (1, 4, 64, 4, 0)])
def test_bad_arguments_are_invalid(host, args):
    assert _entry(host, *args) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().univs_last_error().decode() == ENTRY + ": bad arguments S=%d Ntok=%d E=%d heads=%d Lmax=%d" % args


@pytest.mark.parametrize("null", ("qkv", "start", "out"))
def test_null_pointers_are_invalid(host, null):
    assert _entry(host, 1, 4, 64, 4, 8, null=(null,)) == _lib.ERR_INVALID_ARGUMENT
    assert _lib.load().univs_last_error().decode() == ENTRY + ": NULL data pointer"


@pytest.mark.parametrize("args", [(1, 4, 96, 2, 8),                   # d = 48
                                  (1, 4, 256, 2, 8),                  # d = 128
                                  (1, 4, 64, 8, 8),                   # d = 8
                                  (1, 129, 64, 4, 129),               # a length of 129
                                  (1, 2 ** 31 // 192 + 1, 64, 4, 8),  # Ntok 3 E = 2^31 + 128
                                  (2 ** 29, 4, 64, 4, 8)])            # S heads = 2^31
def test_beyond_each_bound_the_entry_answers_not_implemented_before_any_launch(host, args):
    assert _entry(host, *args) == _lib.ERR_NOT_IMPLEMENTED, args
    assert _lib.load().univs_last_error().decode() == NOT_COVERED


def test_nothing_to_do_is_success_without_a_launch():
    assert _entry(None, 0, 4, 64, 4, 8) == _lib.OK and _entry(None, 3, 0, 64, 4, 8) == _lib.OK


@pytest.mark.parametrize("start,why", [([0, 3, 2, 5], "decreasing"), ([0, 2, 4], "last entry"), ([0, 5], "Lmax"), ([1, 5], "first"),
                                       ([], "S + 1")])
def test_a_wrong_row_table_raises_before_anything_else(start, why):
    qkv = torch.zeros((5, 3 * 64))
    with pytest.raises(ValueError, match="start:"):
        text_ops.varlen_causal_attention(qkv, start, 4, 4)              # (a CPU tensor: the table is looked at first)
    with pytest.raises(ValueError, match="start:"):
        text_ops.varlen_causal_attention_aten(qkv, start, 4, 4)
    with pytest.raises(ValueError, match="start:"):
        text_ops.check_start(torch.tensor(start, dtype=torch.int32), 5, 4)


def test_wrapper_refuses_cpu_tensors_and_odd_arguments():
    with pytest.raises(RuntimeError) as e:
        text_ops.varlen_causal_attention(torch.zeros((5, 3 * 64)), [0, 2, 5], 4, 4)
    assert str(e.value) == str(ops._cpu_refusal("varlen_causal_attention", "tensor on cpu"))
    for bad in (torch.zeros((5, 3 * 64), dtype=torch.float64), torch.zeros((5, 100)), torch.zeros((5, 3, 64))):
        with pytest.raises(RuntimeError, match="float32 qkv"):
            text_ops.varlen_causal_attention(bad, [0, 2, 5], 4, 4)
    with pytest.raises(RuntimeError, match="float32 qkv"):
        text_ops.varlen_causal_attention(torch.zeros((5, 3 * 64)), [0, 2, 5], 5, 4)   # heads does not divide E
    assert not hasattr(ops, "varlen_causal_attention")                   # (ops.py's public set is pinned)


def test_aten_formulation_follows_the_rule_on_the_cpu():
    lengths = [1, 2, 9, 64, 65, 77, 5, 0, 128]
    start = [0]
    for n in lengths:
        start.append(start[-1] + n)
    h, d = 3, 16
    qkv = torch.randn((start[-1], 3 * h * d), generator=torch.Generator().manual_seed(2))
    got = text_ops.varlen_causal_attention_aten(qkv, start, h, 128, dtype=torch.float64)
    for a, b in zip(start[:-1], start[1:]):
        if a == b:
            continue
        q, k, v = qkv[a:b].double().view(b - a, 3, h, d).permute(1, 2, 0, 3)
        s = (q @ k.transpose(-1, -2) / math.sqrt(d)).masked_fill(torch.ones(b - a, b - a, dtype=torch.bool).triu_(1), float("-inf"))
        ref = (s.softmax(-1) @ v).transpose(0, 1).reshape(b - a, h * d)
        assert (got[a:b] - ref).abs().max().item() < 1e-12
    assert (text_ops.varlen_causal_attention_aten(qkv, start, h, 128) - got.float()).abs().max().item() < 2e-5
