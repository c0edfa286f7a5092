"""What vps_eval_bench.py, vss_eval_bench.py and davis_eval_bench.py share: the command line's common part, the kernel-versus-ATen
measurement on one GPU, the timed host-side loop, and the one JSON line.  A tool keeps its scene, its tree writer, its numpy restatement
of the reference and the keys that only it prints."""
import argparse
import json
import os
import statistics
import time

import torch


def arg_parser(reps):
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=reps)
    ap.add_argument("--out", default=None)
    return ap


def gpu_or_exit(tool):
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: no GPU; a timing anywhere else says nothing")
    return torch.device("cuda")


def stats(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def sample(fn, reps):
    """Microseconds per call: the synchronised wall time of `reps` back-to-back calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def kernel_vs_aten(out, args, kernel, aten, equal_key, algorithmic_bytes=None):
    """kernel_us and aten_us into `out`: `args.warmup` untimed calls of each side, then `args.samples` samples, alternating; a kernel
    sample is `args.reps` calls, an ATen sample one.  Then kernel_GBps when the bytes are given, `equal_key` (every tensor of the two
    results equal) and kernel_faster_beyond_spread = max(kernel) < min(aten).  aten=None: the kernel alone."""
    sides = [("kernel", kernel, args.reps)] + ([("aten", aten, 1)] if aten else [])
    for _ in range(args.warmup):
        for _, fn, _ in sides:
            fn()
    us = {k: [] for k, _, _ in sides}
    for _ in range(args.samples):
        for k, fn, reps in sides:
            us[k].append(sample(fn, reps))
    for k in us:
        out[f"{k}_us"] = stats(us[k])
    if algorithmic_bytes:
        out["kernel_GBps"] = round(algorithmic_bytes / (out["kernel_us"]["median"] * 1e-6) / 1e9, 1)
    if aten:
        out[equal_key] = bool(all(torch.equal(x, y) for x, y in zip(kernel(), aten())))
        out["kernel_faster_beyond_spread"] = out["kernel_us"]["max"] < out["aten_us"]["min"]


def timed(fn, warmup, samples):
    """(the seconds of `samples` calls of the host-side `fn` after `warmup` untimed ones, the last call's result)"""
    s, r = [], None
    for i in range(warmup + samples):
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        if i >= warmup:
            s.append(t1 - t0)
    return s, r


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
