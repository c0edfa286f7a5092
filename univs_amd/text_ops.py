"""Wrappers of the eighteenth header (include/univs_text_hip.h): causal self-attention over packed sequences of unequal length.

  check_start                    the row table of a packed batch, checked on the host where it was built -> int32 [S + 1] (CPU)
  varlen_causal_attention        out [Ntok, E] of qkv [Ntok, 3 E] by the kernel (csrc/text_attn.hip); None beyond its coverage
  varlen_causal_attention_aten   the same rule in torch: sequences padded per length bucket, torch softmax -- the fallback beyond the
                                 kernel's coverage, the CPU path, and the yardstick

The kernel wrapper runs behind `ops._call`: GPU tensors only (a CPU tensor raises), None where the kernel does not cover the call.
"""
import math

import torch

from . import _lib, ops

MAX_LEN = 128                    # keys of a sequence: two per lane
HEAD_DIMS = (16, 32, 64)


def check_start(start, Ntok, Lmax):
    """`start` (a sequence of ints or a CPU integer tensor, S + 1 entries) as int32 [S + 1] on the CPU, after the checks the kernel cannot
    report: first entry 0, non-decreasing, last entry Ntok, every length <= Lmax.  The table is built from host lengths, so this costs no
    download; a tensor on a device is refused for that reason."""
    if isinstance(start, torch.Tensor):
        if start.is_cuda:
            raise ValueError("start: the row table is checked on the host; pass the host copy it was built from")
        t = start.detach().reshape(-1).to(torch.int64)
    else:
        t = torch.as_tensor(list(start), dtype=torch.int64)
    if t.numel() < 1 or int(t[0]) != 0:
        raise ValueError("start: S + 1 entries, the first one 0")
    if int(t[-1]) != int(Ntok):
        raise ValueError(f"start: the last entry is {int(t[-1])}, qkv has {int(Ntok)} rows")
    lengths = t[1:] - t[:-1]
    if lengths.numel() and int(lengths.min()) < 0:
        raise ValueError("start: decreasing")
    if lengths.numel() and int(lengths.max()) > int(Lmax):
        raise ValueError(f"start: a sequence of {int(lengths.max())} rows, Lmax={int(Lmax)}")
    return t.to(torch.int32)


def _check_qkv(name, qkv, heads, Lmax):
    h, Lmax = int(heads), int(Lmax)
    if qkv.dtype != torch.float32 or qkv.dim() != 2 or qkv.shape[1] % 3 or h < 1 or Lmax < 1 or (qkv.shape[1] // 3) % h or qkv.shape[1] == 0:
        raise RuntimeError(f"{name}: float32 qkv [Ntok, 3 E] with heads | E and Lmax >= 1, got {qkv.dtype} {tuple(qkv.shape)} heads={h} Lmax={Lmax}")
    return int(qkv.shape[0]), int(qkv.shape[1]) // 3, h, Lmax


def varlen_causal_attention(qkv, start, heads, Lmax, start_dev=None, out=None):
    """out [Ntok, E]: row i of a sequence is softmax(q_i . k_{j <= i} / sqrt(d)) v_{j <= i} per head, on qkv's device and current stream.
    `start`: the host row table (check_start raises on a wrong one); `start_dev`: its int32 copy on qkv's device where the caller already
    uploaded it (the tower uses one table for all its blocks), uploaded here otherwise.  `out`: a contiguous float32 [Ntok, E] on qkv's
    device to write into (allocated here otherwise); only the rows of the sequences are written.
    None beyond d in {16, 32, 64}, Lmax <= 128, Ntok 3 E < 2^31: the caller keeps `varlen_causal_attention_aten`."""
    name = "varlen_causal_attention"
    ops._inference_only(name, qkv)
    Ntok, E, h, Lmax = _check_qkv(name, qkv, heads, Lmax)
    table = check_start(start, Ntok, Lmax)
    ops._require_gpu(name, qkv)
    S = table.numel() - 1
    if E // h not in HEAD_DIMS or Lmax > MAX_LEN or Ntok * 3 * E >= 2 ** 31 or S * h >= 2 ** 31:
        return None                                                  # (the entry's answer, without allocating what it would not write)
    if start_dev is None:
        start_dev = table.to(qkv.device)
    elif start_dev.dtype != torch.int32 or start_dev.device != qkv.device or start_dev.numel() != S + 1 or not start_dev.is_contiguous():
        raise RuntimeError(f"{name}: start_dev has to be the contiguous int32 [{S + 1}] copy of start on {qkv.device}")
    if out is None:
        out = torch.empty((Ntok, E), dtype=torch.float32, device=qkv.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (Ntok, E) or out.device != qkv.device or not out.is_contiguous():
        raise RuntimeError(f"{name}: out has to be a contiguous float32 [{Ntok}, {E}] on {qkv.device}")
    if S == 0 or Ntok == 0:
        return out
    ok = ops._call(name, _lib.load().univs_text_attention_f32, qkv, ops._ptr(qkv), ops._ptr(start_dev), S, Ntok, E, h, Lmax,
                   1.0 / math.sqrt(E // h), ops._ptr(out))
    return out if ok else None


def _bucket(n):
    """The padded length of a sequence of n rows: the next power of two, 8 at least."""
    return max(8, 1 << (int(n) - 1).bit_length())


def varlen_causal_attention_aten(qkv, start, heads, Lmax, dtype=None):
    """The same rule from torch's matmul and softmax on any device: the sequences of one length bucket are padded to its length (their
    last row repeated: under the causal mask no kept row attends to the padding) and run as one batch.  `dtype`: the arithmetic's
    (torch.float64: the tests' yardstick); the result comes back in it."""
    name = "varlen_causal_attention_aten"
    Ntok, E, h, Lmax = _check_qkv(name, qkv, heads, Lmax)
    table = check_start(start, Ntok, Lmax).to(torch.int64)
    d = E // h
    x = qkv if dtype is None else qkv.to(dtype)
    out = torch.zeros((Ntok, E), dtype=x.dtype, device=x.device)
    lengths = table[1:] - table[:-1]
    buckets = {}
    for s, n in enumerate(lengths.tolist()):
        if n > 0:
            buckets.setdefault(_bucket(n), []).append(s)
    for Lb, seqs in sorted(buckets.items()):
        idx = torch.as_tensor(seqs)
        first, n = table[idx], lengths[idx]                                              # [B]
        t = torch.arange(Lb)
        rows = (first[:, None] + torch.minimum(t[None, :], n[:, None] - 1)).to(x.device)  # [B, Lb]
        keep = (t[None, :] < n[:, None]).to(x.device)
        q, k, v = x[rows].view(len(seqs), Lb, 3, h, d).permute(2, 0, 3, 1, 4)            # [B, h, Lb, d] each
        scores = torch.matmul(q * (1.0 / math.sqrt(d)), k.transpose(-1, -2))
        scores = scores.masked_fill(torch.ones(Lb, Lb, dtype=torch.bool, device=x.device).triu_(1), float("-inf"))
        o = torch.matmul(torch.softmax(scores, dim=-1), v).permute(0, 2, 1, 3).reshape(len(seqs), Lb, E)
        out[rows[keep]] = o[keep]
    return out
