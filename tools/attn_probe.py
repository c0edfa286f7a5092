"""The attention cores alone, at the shapes of BASELINE config 2 (Swin-T, T = 5 @ 736 x 1280, 100 queries): the three cross-attention
levels, the decoder's self-attention over Q' T = 500 tokens, and the stage-1 / stage-2 window attention.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES -d out -- python tools/attn_probe.py --reps 3 --no-time
    python tools/pmc_summary.py out xattn_partial,window_attn_img
    python tools/attn_probe.py --sweep          # cross-attention: us per launch pair (partial + merge) by (segments, query blocks per wave)

A counter pass runs on its own, with no tracing beside it.  `--sweep` forces the launch choice through UnivsConfig.xattn_segments
(segments + 65536 x query blocks per wave, see csrc/cross_attn.hip); 0 / 0 is the library's own choice."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from univs_amd import ops, synth  # noqa: E402

XATTN = (("1/8", 100, 14720, 5, 8, True), ("1/16", 100, 3680, 5, 8, True), ("1/32", 100, 920, 5, 8, True), ("self", 500, 500, 1, 8, False))
WINDOW = (("stage 1", 5, 184, 320, 7, 3, 3), ("stage 2", 5, 92, 160, 7, 3, 6))


def xattn_args(L, S, N, H, masked, dev):
    E = 32 * H
    q = synth.normal(f"probe/q/{L}x{N}", (L, N, E)).to(dev)
    k = synth.normal(f"probe/k/{S}x{N}", (S, N, E)).to(dev)
    v = synth.normal(f"probe/v/{S}x{N}", (S, N, E)).to(dev)
    mask = None
    if masked:
        mask = (torch.rand(N, L, S, generator=torch.Generator().manual_seed(S)) < 0.6).to(dev)
    return q, k, v, mask, H, 32 ** -0.5


def window_args(B, H, W, ws, shift, nH, dev):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from record_attn_bits import window_inputs
    qkv, qb, bias, mask = window_inputs(B, H, W, ws, shift, nH)
    return qkv.to(dev), qb.to(dev), bias.to(dev), mask.to(dev), H, W, ws, shift, 32 ** -0.5


def timed(fn, reps):
    """us per call, device time: `reps` calls captured into one graph (a chain: no host time between the launches), best of 3 replays"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(3):
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-time", action="store_true", help="launch only (counter passes)")
    ap.add_argument("--segments", default="0,3,5,8,9,10,12,15,16,19,23,26,29,32,39,46,51")
    ap.add_argument("--blocks", default="0,1,2,3,4,7")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    xs = [(name, L, S, N, H, xattn_args(L, S, N, H, m, dev)) for name, L, S, N, H, m in XATTN]
    if args.sweep:
        for name, L, S, N, H, a in xs:
            nit = (S + 31) // 32
            for nqb in (int(x) for x in args.blocks.split(",")):
                if nqb > (min(L, 128) + 15) // 16:
                    continue
                for seg in (int(x) for x in args.segments.split(",")):
                    if seg > nit or (seg == 0) != (nqb == 0):
                        continue
                    with ops.configured(xattn_segments=seg + 65536 * nqb):
                        us = timed(lambda: ops.cross_attention(*a), 20)
                    print(f"xattn {name:5s} L={L} S={S} N={N} H={H}  segments={seg:3d} blocks={nqb}  {us:8.1f} us", flush=True)
        return
    ws = [(name, window_args(B, H, W, wsz, shift, nH, dev)) for name, B, H, W, wsz, shift, nH in WINDOW]
    for _ in range(args.reps):
        for name, L, S, N, H, a in xs:
            ops.cross_attention(*a)
        for name, a in ws:
            ops.window_attention_image(*a, mma="f16x3")
    torch.cuda.synchronize()
    if args.no_time:
        return
    for name, L, S, N, H, a in xs:
        print(f"xattn {name:5s} L={L} S={S} N={N} H={H}  {timed(lambda: ops.cross_attention(*a), 20):8.1f} us (partial + merge, back to back)")
    for name, a in ws:
        print(f"window {name}  {timed(lambda: ops.window_attention_image(*a, mma='f16x3'), 20):8.1f} us")


if __name__ == "__main__":
    main()
