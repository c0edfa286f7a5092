"""Scoring one synthetic VIPOSeg-shaped video four ways: 20 frames at 720 x 1280 (d = 29) with 30 tracked objects; 4 frames at
120 x 214 with 6 objects with --quick.  Prints one JSON line and writes it to --out.

  kernel_us / aten_us       the counts of the video (both uint8 stacks already on the device) from csrc/pvos_count.hip and from
                            `pvos_counts_aten` on the same GPU: median, min and max over `--samples` samples after `--warmup` untimed
                            ones, alternating; a sample is the synchronised wall time of `--reps` back-to-back kernel calls (one ATen
                            call), the output allocation of the wrapper included
  kernel_peak_bytes / aten_peak_bytes   the peak of the allocator during one call above the two input stacks and the output
  evaluate_files_s          the whole `evaluate_pvos_files` on the video's tree, with the decay: every PNG decoded once, one upload,
                            one launch, the host arithmetic
  numpy_reference_s_per_frame  the reference's loop restated in numpy + SciPy on the same host from its description, on the first
                            `--ref_frames` frames only (it is slow), per frame: for every tracked object the two masks, the zero border,
                            d erosions by 3 x 3 of each, the six sums.  This is NO timing of OpenCV, whose erosion the reference calls
  evaluate_files_s_per_frame   evaluate_files_s over the number of frames, for the comparison with the line above

The yardstick of the kernel is the ATen formulation in the same run: `kernel_faster_beyond_spread` is max(kernel) < min(aten).

    python tools/pvos_eval_bench.py [--quick] [--samples 5] [--warmup 2] [--reps 10] [--out profiles/pvos_eval_bench_v1.json]
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eval_bench_common as bench                         # noqa: E402
from univs_amd.evaluation import pvos                     # noqa: E402
from univs_amd.evaluation import pvos_counts as pc        # noqa: E402


def scene(T, H, W, K, seed=0):
    """gt: a label map without holes, three bands of stuff (ids 1..3) under K - 3 ellipses that move and breathe; result: the same a few
    pixels off, 0.05 % single-pixel errors."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    objs = [(rng.uniform(0.1, 0.9) * H, rng.uniform(0.1, 0.9) * W, rng.uniform(0.04, 0.12) * H, rng.uniform(0.03, 0.1) * W,
             rng.uniform(-0.004, 0.004) * H, rng.uniform(-0.006, 0.006) * W) for _ in range(K - 3)]
    gt, pred = np.zeros((T, H, W), np.uint8), np.zeros((T, H, W), np.uint8)
    for t in range(T):
        for m, off in ((gt, 0.0), (pred, 0.004)):
            m[t, : H // 3], m[t, H // 3: int(H * (0.6 + off))], m[t, int(H * (0.6 + off)):] = 1, 2, 3
            for k, (cy, cx, ry, rx, vy, vx) in enumerate(objs):
                a, b = ry * (1 + 0.1 * np.sin(0.3 * t + k)) * (1 + 6 * off), rx * (1 + 0.1 * np.cos(0.2 * t + k)) * (1 - 4 * off)
                m[t][((yy - cy - vy * t - off * H) / a) ** 2 + ((xx - cx - vx * t + off * W) / b) ** 2 <= 1] = k + 4
        noise = rng.random((H, W)) < 0.0005
        pred[t][noise] = (pred[t][noise] % K) + 1
    return gt, pred


def write_tree(root, gt, pred, K):
    from PIL import Image
    data, res = os.path.join(root, "valid"), os.path.join(root, "Annotations")
    for sub, m in ((os.path.join(data, "Annotations_gt", "v"), gt), (os.path.join(res, "v"), pred), (os.path.join(data, "Annotations", "v"), gt[:1])):
        os.makedirs(sub, exist_ok=True)
        for t in range(len(m)):
            Image.fromarray(m[t]).save(os.path.join(sub, "%05d.png" % t))
    with open(os.path.join(data, "obj_class.json"), "w") as f:
        json.dump({"v": {str(k): (pvos.STUFF_SEEN_CLASS[0] if k <= 3 else pvos.THING_SEEN_CLASS[0]) for k in range(1, K + 1)}}, f)
    return data, res


def numpy_reference(gt, pred, K, d):
    """The six counts [T, K, 6] as the reference's loop gets them: per object and frame, two padded masks eroded d times."""
    from scipy.ndimage import binary_erosion
    T, H, W = gt.shape
    ones = np.ones((3, 3), np.uint8)

    def boundary(mask):
        eroded = binary_erosion(np.pad(mask, 1, constant_values=0), structure=ones, iterations=d, border_value=1).astype(np.uint8)
        return mask - eroded[1:H + 1, 1:W + 1]
    out = np.zeros((T, K, 6), np.int64)
    for t in range(T):
        for k in range(1, K + 1):
            g, p = gt[t] == k, pred[t] == k
            gb, pb = boundary(g.astype(np.uint8)), boundary(p.astype(np.uint8))
            out[t, k - 1] = (np.sum(g & p), np.sum(g), np.sum(p), ((gb * pb) > 0).sum(), (gb > 0).sum(), (pb > 0).sum())
    return out


def peak_bytes(fn):
    """The allocator's peak during `fn()` above what was allocated before it and the tensor it returns."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base - r.numel() * r.element_size())


def one(T, H, W, K, args, dev):
    d = pc.dilation(H, W)
    gt, pred = scene(T, H, W, K)
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    out = {"frames": T, "size": [H, W], "objects": K, "d": d}
    bench.kernel_vs_aten(out, args, lambda: pc.pvos_video_counts(g, p, d, K), lambda: pc.pvos_counts_aten(g, p, d, K), "counts_equal",
                         algorithmic_bytes=2 * T * H * W)
    out["kernel_peak_bytes"] = peak_bytes(lambda: pc.pvos_video_counts(g, p, d, K))
    out["aten_peak_bytes"] = peak_bytes(lambda: pc.pvos_counts_aten(g, p, d, K))
    torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as root:
        data, res = write_tree(root, gt, pred, K)
        ev, _ = bench.timed(lambda: pvos.evaluate_pvos_files(res, data, eval_decay=True, device=dev), args.warmup, args.samples)
    n = min(T, args.ref_frames)
    ref, counts = bench.timed(lambda: numpy_reference(gt[:n], pred[:n], K, d), 0, 2)
    out["reference_counts_equal"] = bool(np.array_equal(counts, pc.pvos_counts(g[:n].contiguous(), p[:n].contiguous(), d, K).cpu().numpy()))
    out["evaluate_files_s"] = bench.stats(ev, 3)
    out["evaluate_files_s_per_frame"] = bench.stats([v / T for v in ev], 4)
    out["numpy_reference_frames"] = n
    out["numpy_reference_s_per_frame"] = bench.stats([v / n for v in ref], 3)
    out["evaluate_faster_beyond_spread"] = out["evaluate_files_s_per_frame"]["max"] < out["numpy_reference_s_per_frame"]["min"]
    return out


def main():
    ap = bench.arg_parser(reps=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ref_frames", type=int, default=1)
    args = ap.parse_args()
    dev = bench.gpu_or_exit("pvos_eval_bench")
    cases = [(4, 120, 214, 6)] if args.quick else [(20, 720, 1280, 30)]
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "reps": args.reps, "sequences": []}
    for c in cases:
        out["sequences"].append(one(*c, args, dev))
        print(json.dumps(out["sequences"][-1]), file=sys.stderr, flush=True)
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
