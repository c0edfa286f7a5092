"""SHA-256 of what the attention cores (csrc/cross_attn.hip, csrc/window_attn_f16.hip) return for seeded inputs.

    python tools/record_attn_bits.py [--out tests/golden/attn_parent_bits.json]

Run on the GPU with the library of the commit whose bits are to be kept (UNIVS_HIP_LIB names another build of it); the file it
writes is what tests/test_attention_bits_gpu.py requires of every later tree: an instruction-level rewrite of the two kernels keeps
every bit.  The cross-attention cases force three key segments (UnivsConfig.xattn_segments), so the merge's order of summation is
part of the record.  The cases are defined here, once; the test imports them from this file."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from univs_amd import ops, synth  # noqa: E402

SEGMENTS = 3
# name -> (L, S, N, H, kind): "flags" a DeferredMask (byte mask + generation flags, one all-masked row whose flag is stale),
# "mask" a bool [N, L, S] mask, "none" unmasked, "mask2d" one [L, S] mask for the one batch entry (the decoder's self-attention),
# "ranges" = "flags" with one K block at 2^16, one V block at 1e-6 and one all-zero V block
XATTN_CASES = {
    "xattn_100x920x5x8_flags": (100, 920, 5, 8, "flags"),
    "xattn_7x33x1x1_mask": (7, 33, 1, 1, "mask"),
    "xattn_130x64x2x2_none": (130, 64, 2, 2, "none"),
    "xattn_500x500x1x8_mask2d": (500, 500, 1, 8, "mask2d"),
    "xattn_100x920x5x8_ranges": (100, 920, 5, 8, "ranges"),
}
# name -> (B, H, W, ws, shift, nH, mma)
WINDOW_CASES = {f"window_{B}x{H}x{W}_ws{ws}_s{shift}_h{nH}_{mma}": (B, H, W, ws, shift, nH, mma)
                for mma in ("f16x3", "f16")
                for (B, H, W, ws, shift, nH) in ((2, 16, 16, 7, 0, 3), (2, 16, 16, 7, 3, 3), (1, 24, 24, 12, 6, 4))}


def xattn_inputs(name, rows=None):
    """(q, k, v, mask) on the CPU; mask is None, a bool tensor, or (bytes uint8 [N, L, S], flags int32 [N * L], generation).
    `rows`: only the first `rows` queries (the same values as those rows of the full case)."""
    L, S, N, H, kind = XATTN_CASES[name]
    E = 32 * H
    q = synth.normal(f"attn_bits/q/{L}x{N}x{E}", (L, N, E))
    k = synth.normal(f"attn_bits/k/{S}x{N}x{E}", (S, N, E))
    v = synth.normal(f"attn_bits/v/{S}x{N}x{E}", (S, N, E))
    mask = None
    if kind != "none":
        m = synth.uniform(f"attn_bits/m/{N}x{L}x{S}", (N, L, S)) > -0.2          # 60 % masked
        m[:, 1::5, : S // 2] = True                                               # whole segments masked for some queries
        if S > 128:
            m[:, 2::7, 64:128] = True                                            # whole 32-key iterations
        m[..., S - 1] = False                                                     # no row without a visible key ...
        if kind in ("flags", "ranges"):
            gen = 7
            flags = torch.full((N, L), gen, dtype=torch.int32)
            m[0, 3] = True                                                        # ... but this one, whose flag is stale: every key visible
            flags[0, 3] = gen - 1
            flags[N - 1, L - 1] = 0                                               # (and one ordinary row that does not count)
            mask = (m.to(torch.uint8), flags.reshape(-1), gen)
        else:
            mask = m
    if kind == "ranges":
        k[64:96] *= 65536.0
        v[128:160] *= 1.0e-6
        v[192:224] = 0.0
    if rows is not None:
        q = q[:rows].contiguous()
        if isinstance(mask, tuple):
            mask = (mask[0][:, :rows].contiguous(), mask[1].reshape(N, L)[:, :rows].reshape(-1).contiguous(), mask[2])
        elif mask is not None:
            mask = mask[:, :rows].contiguous()
    return q, k, v, mask


def run_xattn(name, device, segments=SEGMENTS, rows=None):
    H = XATTN_CASES[name][3]
    q, k, v, mask = xattn_inputs(name, rows)
    if isinstance(mask, tuple):
        mask = ops.DeferredMask(mask[0].to(device), mask[1].to(device), mask[2])
    elif mask is not None:
        mask = mask.to(device)
    with ops.configured(xattn_segments=segments):
        out = ops.cross_attention(q.to(device), k.to(device), v.to(device), mask, H, 32 ** -0.5)
    assert out is not None, name
    return out


def window_inputs(B, H, W, ws, shift, nH):
    n = ws * ws
    tag = f"attn_bits/w/{B}/{H}/{W}/{ws}/{shift}/{nH}"
    qkv = synth.normal(tag + "/qkv", (B, H * W, 3, nH, 32))
    qb = synth.normal(tag + "/qb", (3 * nH * 32,)) * 0.5
    bias = synth.normal(tag + "/bias", (nH, n, n))
    Hp, Wp = (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws
    mask = None
    if shift:                                                    # the shift mask of swin.py:413-440: region ids on the padded canvas -> 0 / -100
        img = torch.zeros(1, Hp, Wp, 1)
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[:, hs, wsl, :] = cnt
                cnt += 1
        mw = img.view(1, Hp // ws, ws, Wp // ws, ws, 1).permute(0, 1, 3, 2, 4, 5).reshape(-1, n)
        am = mw.unsqueeze(1) - mw.unsqueeze(2)
        mask = am.masked_fill(am != 0, -100.0).masked_fill(am == 0, 0.0)
    return qkv, qb, bias, mask


def run_window(name, device):
    B, H, W, ws, shift, nH, mma = WINDOW_CASES[name]
    qkv, qb, bias, mask = window_inputs(B, H, W, ws, shift, nH)
    return ops.window_attention_image(qkv.to(device), qb.to(device), bias.to(device), mask.to(device) if mask is not None else None,
                                      H, W, ws, shift, 32 ** -0.5, mma=mma)


def digest(t):
    a = t.detach().cpu().contiguous()
    assert torch.isfinite(a).all()
    return hashlib.sha256(a.numpy().tobytes()).hexdigest()


def record(device):
    out = {}
    for name in XATTN_CASES:
        out[name] = digest(run_xattn(name, device))
    for name in WINDOW_CASES:
        out[name] = digest(run_window(name, device))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attn_parent_bits.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    got = record(torch.device("cuda:0"))
    with open(args.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    for n, h in sorted(got.items()):
        print(h[:16], n)


if __name__ == "__main__":
    main()
