"""The resampling step of the semantic-extraction driver at three shipped-like geometries, fused (csrc/semantic_extract.hip through
video_semantic_extraction.FusedSteps) against the ATen formulation of the same step (AtenSteps: the reference's F.interpolate(bilinear)
to the padded size, crop, F.interpolate(nearest)) in the same process, alternating.  Prints one JSON line:

  720p_r8     five 736 x 1280 padded frames (720 x 1280 image and output), mask features [5, 256, 184, 320], ratio 8  -> [5, 256, 90, 160]
  720p_r32    the same clip at the default ratio 32                                                                  -> [5, 256, 22, 40]
  lsj_r32     five frames under the 1024 x 1024 LSJ square (576 x 1024 image, 720 x 1280 output), features [5, 256, 256, 256],
              ratio 32                                                                                               -> [5, 256, 22, 40]
  *_fused_us / *_aten_us   median, min and max of the time per call over `--samples` samples after `--warmup` untimed ones; a sample is
                           the synchronised wall time of `--reps` back-to-back fused calls (one ATen call) divided by the calls
  *_peak_bytes             torch.cuda.max_memory_allocated during one call, above what was allocated before it
  *_algorithmic_bytes      what the gather has to move: the 128-byte lines of the input it touches plus the output
  *_fused_GBps             algorithmic bytes over the median fused time (a host clock around back-to-back launches: it includes the
                           launch overhead; the kernel's own time is in the rocprofv3 trace)
  *_max_abs_diff           fused against ATen on the device

    python tools/semantic_bench.py [--samples 5] [--warmup 2] [--reps 50] [--only NAME] [--fused-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from univs_amd.inference.image_generic_seg import nearest_source_index                       # noqa: E402
from univs_amd.inference.video_semantic_extraction import AtenSteps, FusedSteps              # noqa: E402

GEOMETRY = {
    "720p_r8": dict(x=(5, 256, 184, 320), padded=(736, 1280), crop=(720, 1280), out=(720, 1280), ratio=8),
    "720p_r32": dict(x=(5, 256, 184, 320), padded=(736, 1280), crop=(720, 1280), out=(720, 1280), ratio=32),
    "lsj_r32": dict(x=(5, 256, 256, 256), padded=(1024, 1024), crop=(576, 1024), out=(720, 1280), ratio=32),
}
LINE = 128


def size_of(g):
    return int(g["out"][0] / g["ratio"]), int(g["out"][1] / g["ratio"])


def taps(scale, dst, in_size):
    """make_tap of csrc/resample_taps.h on the host: the two source indices of each destination index."""
    src = np.maximum(np.float32(scale) * (dst.astype(np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = src.astype(np.int64)
    return i0, i0 + (i0 < in_size - 1)


def algorithmic_bytes(g):
    """128-byte lines of `in` the gather touches (per plane, times the planes) + the bytes of `out`."""
    T, C, h, w = g["x"]
    hc, wc = size_of(g)
    sy = nearest_source_index(np.arange(hc), g["crop"][0], hc)
    sx = nearest_source_index(np.arange(wc), g["crop"][1], wc)
    ys = np.unique(np.concatenate(taps(np.float32(h) / np.float32(g["padded"][0]), sy, h)))
    xs = np.unique(np.concatenate(taps(np.float32(w) / np.float32(g["padded"][1]), sx, w)))
    lines = np.unique(((ys[:, None] * w + xs[None, :]) * 4) // LINE)
    return int(T * C * (len(lines) * LINE + hc * wc * 4)), int(len(lines) * LINE), h * w * 4


def sample(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def stats(us):
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", choices=list(GEOMETRY), default=None)
    ap.add_argument("--fused-only", action="store_true", help="skip the ATen side (the run under the kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "geometry": GEOMETRY, "samples": args.samples, "reps": args.reps}
    with torch.no_grad():
        for name, g in GEOMETRY.items():
            if args.only not in (None, name):
                continue
            T, C, h, w = g["x"]
            size = size_of(g)
            x = torch.randn(g["x"], device=dev, generator=torch.Generator(device=dev).manual_seed(0))
            bufs = {k: torch.empty((T, C) + size, device=dev) for k in ("fused", "aten")}
            fused = lambda: FusedSteps(g["padded"], g["crop"], size).compress(x, 0, 1, bufs["fused"])
            aten = lambda: AtenSteps(g["padded"], g["crop"], size).compress(x, 0, 1, bufs["aten"])
            sides = [("fused", fused, args.reps)] + ([] if args.fused_only else [("aten", aten, 1)])
            for _ in range(args.warmup):
                for _, fn, _ in sides:
                    fn()
            torch.cuda.synchronize()
            us = {k: [] for k, _, _ in sides}
            for _ in range(args.samples):                      # alternating: both sides see the same neighbours
                for k, fn, reps in sides:
                    us[k].append(sample(fn, reps))
            for k, fn, _ in sides:
                out[f"{name}_{k}_us"] = stats(us[k])
                out[f"{name}_{k}_peak_bytes"] = peak(fn)
            total, lines_per_plane, plane = algorithmic_bytes(g)
            out[f"{name}_out_shape"] = [T, C, *size]
            out[f"{name}_stack_bytes"] = T * C * g["padded"][0] * g["padded"][1] * 4
            out[f"{name}_algorithmic_bytes"] = total
            out[f"{name}_input_line_bytes_per_plane"] = [lines_per_plane, plane]
            out[f"{name}_fused_GBps"] = round(total / (out[f"{name}_fused_us"]["median"] * 1e-6) / 1e9, 1)
            if not args.fused_only:
                out[f"{name}_max_abs_diff"] = float((bufs["fused"] - bufs["aten"]).abs().max())
                out[f"{name}_speedup"] = round(out[f"{name}_aten_us"]["median"] / out[f"{name}_fused_us"]["median"], 1)
                out[f"{name}_faster_beyond_spread"] = out[f"{name}_fused_us"]["max"] < out[f"{name}_aten_us"]["min"]
            del x, bufs
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
