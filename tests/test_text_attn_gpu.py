"""GPU: causal attention over packed sequences of unequal length (csrc/text_attn.hip, text_ops.varlen_causal_attention) against a float64
torch formulation on N(0, 1) inputs.  Bound: max-abs below 2e-5, the bound of the project's fp32 attention cores (tests/test_ops_gpu.py:
window core and cross-attention)."""
import math

import pytest
import torch

from univs_amd import text_ops

pytestmark = pytest.mark.gpu

TOL = 2e-5
MIXED = [1, 2, 63, 64, 65, 77, 128, 3, 5, 9, 4, 13, 1, 7]        # every edge of the two-keys-per-lane layout, and several short ones


def starts(lengths):
    s = [0]
    for n in lengths:
        s.append(s[-1] + n)
    return s


def reference(qkv, start, heads):
    """float64, one sequence at a time: softmax(q k^T / sqrt(d) + triu(-inf)) v."""
    x = qkv.double().cpu()
    E = x.shape[1] // 3
    d = E // heads
    out = torch.zeros((x.shape[0], E), dtype=torch.float64)
    for a, b in zip(start[:-1], start[1:]):
        n = b - a
        if n == 0:
            continue
        q, k, v = x[a:b].view(n, 3, heads, d).permute(1, 2, 0, 3)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(d)
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool).triu_(1), float("-inf"))
        out[a:b] = (s.softmax(-1) @ v).transpose(0, 1).reshape(n, E)
    return out


def qkv_of(lengths, heads, d, cuda, seed=0):
    gen = torch.Generator().manual_seed(seed + 1000 * heads + d)
    return torch.randn((sum(lengths), 3 * heads * d), generator=gen).to(cuda)


@pytest.mark.parametrize("heads", [1, 4, 10])
@pytest.mark.parametrize("d", [16, 32, 64])
def test_mixed_lengths_match_float64(cuda, d, heads):
    start = starts(MIXED)
    qkv = qkv_of(MIXED, heads, d, cuda)
    got = text_ops.varlen_causal_attention(qkv, start, heads, 128)
    assert got is not None and got.dtype == torch.float32 and tuple(got.shape) == (sum(MIXED), heads * d)
    ref = reference(qkv, start, heads)
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"d={d} heads={heads}: max abs err {err:.2e}")
    assert err < TOL, err
    aten = text_ops.varlen_causal_attention_aten(qkv, start, heads, 128)
    err = (got - aten).abs().max().item()
    assert err < TOL, err


def test_one_sequence_of_one_token_is_its_value(cuda):
    qkv = qkv_of([1], 4, 16, cuda)
    got = text_ops.varlen_causal_attention(qkv, [0, 1], 4, 1)
    assert torch.equal(got, qkv[:, 128:])


@pytest.mark.parametrize("lengths,Lmax", [([7, 11, 13], 13), ([5, 0, 3, 0], 77), ([77] * 3 + [4] * 5, 77)], ids=str)
def test_odd_totals_empty_sequences_and_a_tight_lmax(cuda, lengths, Lmax):
    start = starts(lengths)
    qkv = qkv_of(lengths, 10, 64, cuda, seed=3)
    got = text_ops.varlen_causal_attention(qkv, start, 10, Lmax)
    err = (got.double().cpu() - reference(qkv, start, 10)).abs().max().item()
    assert err < TOL, err


def test_beyond_coverage_is_none(cuda):
    assert text_ops.varlen_causal_attention(torch.zeros((4, 3 * 96), device=cuda), [0, 4], 2, 4) is None          # d = 48
    assert text_ops.varlen_causal_attention(torch.zeros((129, 3 * 64), device=cuda), [0, 129], 4, 129) is None    # a length of 129
    assert text_ops.varlen_causal_attention(torch.zeros((4, 3 * 256), device=cuda), [0, 4], 2, 4) is None         # d = 128


def test_guard_rows_around_out_stay_untouched(cuda):
    """`out` is the middle of a poisoned buffer: the rows in front of it and behind it keep the poison."""
    lengths, heads, d = [65, 3, 128, 1], 4, 32
    E, Ntok, guard = heads * d, sum(lengths), 64
    qkv = qkv_of(lengths, heads, d, cuda, seed=5)
    buf = torch.full((Ntok + 2 * guard, E), 12345.0, device=cuda)
    got = text_ops.varlen_causal_attention(qkv, starts(lengths), heads, 128, out=buf[guard:guard + Ntok])
    assert got.data_ptr() == buf[guard].data_ptr()
    with pytest.raises(RuntimeError, match="out has to be"):
        text_ops.varlen_causal_attention(qkv, starts(lengths), heads, 128, out=buf[:Ntok, :E - 1])
    assert bool((buf[:guard] == 12345.0).all()) and bool((buf[guard + Ntok:] == 12345.0).all())
    assert (got.double().cpu() - reference(qkv, starts(lengths), heads)).abs().max().item() < TOL
