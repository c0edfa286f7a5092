"""Scoring synthetic DAVIS-shaped sequences four ways: 50 frames at 480 x 854 with 5 objects / 5 proposals (r = 8) and 50 frames at
1080 x 1920 with 3 objects (r = 18); 6 frames at 120 x 214 with --quick.  Prints one JSON line and writes it to --out.  Per sequence:

  kernel_us / aten_us       the counts of the sequence (both uint8 stacks already on the device) from csrc/davis_count.hip and from
                            `davis_counts_aten` on the same GPU: median, min and max over `--samples` samples after `--warmup` untimed
                            ones, alternating; a sample is the synchronised wall time of `--reps` back-to-back kernel calls (one ATen
                            call), the output allocations of the wrapper included
  evaluate_files_s          the whole `evaluate_davis_files` on the sequence's tree (unsupervised task): every PNG decoded once, one
                            upload, one launch, the match, the statistics
  numpy_reference_s_per_frame  the reference's algorithm restated in numpy + SciPy on the same host from its description, on the first
                            `--ref_frames` frames only (it is slow), per frame: for every (gt object, proposal) pair the two boundary
                            maps, two `binary_dilation`s with the disk, the four sums
  evaluate_files_s_per_frame   evaluate_files_s over the number of frames, for the comparison with the line above

The yardstick of the kernel is the ATen formulation in the same run: `kernel_faster_beyond_spread` is max(kernel) < min(aten).

    python tools/davis_eval_bench.py [--quick] [--samples 5] [--warmup 2] [--reps 10] [--out profiles/davis_eval_bench_v1.json]
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eval_bench_common as bench                         # noqa: E402
from univs_amd.evaluation import davis                    # noqa: E402
from univs_amd.evaluation import davis_counts as dc       # noqa: E402


def scene(T, H, W, G, P, seed=0):
    """gt: G ellipses that move and breathe, a void band; result: the same ellipses a few pixels off under permuted ids, 0.05 %
    single-pixel holes."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    objs = [(rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.08, 0.2) * H, rng.uniform(0.06, 0.15) * W,
             rng.uniform(-0.004, 0.004) * H, rng.uniform(-0.006, 0.006) * W) for _ in range(max(G, P))]
    perm = rng.permutation(P)
    gt, pred = np.zeros((T, H, W), np.uint8), np.zeros((T, H, W), np.uint8)
    for t in range(T):
        for k, (cy, cx, ry, rx, vy, vx) in enumerate(objs):
            a, b = ry * (1 + 0.1 * np.sin(0.3 * t + k)), rx * (1 + 0.1 * np.cos(0.2 * t + k))
            if k < G:
                gt[t][((yy - cy - vy * t) / a) ** 2 + ((xx - cx - vx * t) / b) ** 2 <= 1] = k + 1
            if k < P:
                pred[t][((yy - cy - vy * t - 0.004 * H) / (a * 1.03)) ** 2 + ((xx - cx - vx * t + 0.003 * W) / (b * 0.98)) ** 2 <= 1] = perm[k] + 1
        pred[t][rng.random((H, W)) < 0.0005] = 0
    gt[:, :, W // 2:W // 2 + max(2, W // 200)] = 255
    return gt, pred


def write_tree(root, gt, pred):
    from PIL import Image
    d, res = os.path.join(root, "DAVIS"), os.path.join(root, "Annotations")
    for sub, m in ((os.path.join(d, "Annotations_unsupervised", "480p", "v"), gt), (os.path.join(res, "v"), pred)):
        os.makedirs(sub, exist_ok=True)
        for t in range(len(m)):
            Image.fromarray(m[t]).save(os.path.join(sub, "%05d.png" % t))
    os.makedirs(os.path.join(d, "JPEGImages", "480p", "v"))
    for t in range(len(gt)):
        Image.new("RGB", (8, 8)).save(os.path.join(d, "JPEGImages", "480p", "v", "%05d.jpg" % t))
    os.makedirs(os.path.join(d, "ImageSets", "2017"))
    with open(os.path.join(d, "ImageSets", "2017", "val.txt"), "w") as f:
        f.write("v\n")
    return d, res


def numpy_reference(gt, pred, G, P, r):
    """J and F [P, G, T] as the reference computes them: per pair and frame, boundaries and two full-plane dilations."""
    from scipy.ndimage import binary_dilation
    a = np.arange(-r, r + 1)
    disk = a[:, None] ** 2 + a[None, :] ** 2 <= r * r

    def bmap(seg):
        b = np.zeros_like(seg)
        b[:-1, :-1] = (seg[:-1, :-1] ^ seg[:-1, 1:]) | (seg[:-1, :-1] ^ seg[1:, :-1]) | (seg[:-1, :-1] ^ seg[1:, 1:])
        b[-1, :-1] = seg[-1, :-1] ^ seg[-1, 1:]
        b[:-1, -1] = seg[:-1, -1] ^ seg[1:, -1]
        return b
    T = len(gt)
    J, F = np.zeros((P, G, T)), np.zeros((P, G, T))
    void = gt == 255
    for i in range(G):
        for j in range(P):
            for t in range(T):
                g, p = (gt[t] == i + 1) & ~void[t], (pred[t] == j + 1) & ~void[t]
                union = np.sum(g | p)
                J[j, i, t] = np.sum(g & p) / max(union, 1) if union else 1
                gb, pb = bmap(g), bmap(p)
                gd, pd = binary_dilation(gb, structure=disk), binary_dilation(pb, structure=disk)
                n_g, n_p = gb.sum(), pb.sum()
                if n_p == 0 or n_g == 0:
                    pr, rc = (1.0, 1.0) if (n_p == 0 and n_g == 0) else ((1.0, 0.0) if n_p == 0 else (0.0, 1.0))
                else:
                    pr, rc = np.sum(pb & gd) / float(n_p), np.sum(gb & pd) / float(n_g)
                F[j, i, t] = 0 if pr + rc == 0 else 2 * pr * rc / (pr + rc)
    return J, F


def one(T, H, W, G, P, args, dev):
    r = davis.disk_radius(H, W)
    gt, pred = scene(T, H, W, G, P)
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    out = {"frames": T, "size": [H, W], "objects": G, "proposals": P, "radius": r}
    bench.kernel_vs_aten(out, args, lambda: dc.davis_video_counts(g, p, G, P, r, 1), lambda: dc.davis_counts_aten(g, p, G, P, r, 1), "counts_equal")
    torch.cuda.empty_cache()
    with tempfile.TemporaryDirectory() as root:
        d, res = write_tree(root, gt, pred)
        ev, _ = bench.timed(lambda: davis.evaluate_davis_files(d, res, "unsupervised", device=dev), args.warmup, args.samples)
    n = min(T, args.ref_frames)
    ref, (J, F) = bench.timed(lambda: numpy_reference(gt[:n], pred[:n], G, P, r), 0, 2)
    ours = davis.jf_from_counts(*dc.davis_counts(g[:n].contiguous(), p[:n].contiguous(), G, P, r, 1))
    out["scores_equal"] = bool(np.array_equal(J, ours[0].transpose(1, 0, 2)) and np.array_equal(F, ours[1].transpose(1, 0, 2)))
    out["evaluate_files_s"] = bench.stats(ev, 3)
    out["evaluate_files_s_per_frame"] = bench.stats([v / T for v in ev], 4)
    out["numpy_reference_frames"] = n
    out["numpy_reference_s_per_frame"] = bench.stats([v / n for v in ref], 3)
    out["evaluate_faster_beyond_spread"] = out["evaluate_files_s_per_frame"]["max"] < out["numpy_reference_s_per_frame"]["min"]
    return out


def main():
    ap = bench.arg_parser(reps=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ref_frames", type=int, default=2)
    args = ap.parse_args()
    dev = bench.gpu_or_exit("davis_eval_bench")
    cases = [(6, 120, 214, 3, 3)] if args.quick else [(50, 480, 854, 5, 5), (50, 1080, 1920, 3, 3)]
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "reps": args.reps, "sequences": []}
    for c in cases:
        out["sequences"].append(one(*c, args, dev))
        print(json.dumps(out["sequences"][-1]), file=sys.stderr, flush=True)
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
