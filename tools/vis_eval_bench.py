"""Scoring one synthetic YouTube-VIS-shaped video four ways: 36 frames at 720 x 1280 with 100 detections and 10 ground truths
(6 frames at 120 x 214 with 12 and 3 with --quick).  Prints one JSON line and writes it to --out.

  kernel_us / aten_us       the overlap table [D, G, T] of the video (both sides' runs already on the device) from csrc/vis_overlap.hip
                            and from `vis_overlap_aten` on the same GPU: median, min and max over `--samples` samples after `--warmup`
                            untimed ones, alternating; a sample is the synchronised wall time of `--reps` back-to-back kernel calls (one
                            ATen call), the output allocation of the wrapper included
  evaluate_s                `evaluate_predictions_on_ytvis` end to end on the video's annotation and result records: the strings
                            decoded to runs, one upload, one launch, the matching, accumulate, summarize
  numpy_reference_s_per_pair   the reference's `iou_seq` restated in numpy on the same host from its description, on the first
                            `--ref_pairs` (detection, ground truth) pairs only (it is slow), per pair: both masks of every frame decoded,
                            their AND and OR summed
  evaluate_s_per_pair       evaluate_s over D G, for the comparison with the line above

The yardstick of the kernel is the ATen formulation in the same run: `kernel_faster_beyond_spread` is max(kernel) < min(aten).

    python tools/vis_eval_bench.py [--quick] [--samples 5] [--warmup 2] [--reps 10] [--out profiles/vis_eval_bench_v1.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eval_bench_common as bench                         # noqa: E402
from univs_amd.evaluation import vis_counts as vc         # noqa: E402
from univs_amd.evaluation import ytvis                    # noqa: E402
from univs_amd.inference import results as R              # noqa: E402


def scene(T, H, W, D, G, dev, seed=0):
    """(annotation dictionary, result records): G ellipses that move and breathe; D detections, the first G the same ellipses a few
    pixels off, the others elsewhere.  Painted and encoded on the device, one object at a time."""
    rng = np.random.default_rng(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    tt = torch.arange(T, device=dev, dtype=torch.float32)[:, None, None]

    def paint(cy, cx, ry, rx, vy, vx, k):
        a, b = ry * (1 + 0.1 * torch.sin(0.3 * tt + k)), rx * (1 + 0.1 * torch.cos(0.2 * tt + k))
        return ((yy - cy - vy * tt) / a) ** 2 + ((xx - cx - vx * tt) / b) ** 2 <= 1

    def obj():
        return (rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.05, 0.2) * H, rng.uniform(0.04, 0.15) * W,
                rng.uniform(-0.004, 0.004) * H, rng.uniform(-0.006, 0.006) * W)
    objs = [obj() for _ in range(D)]
    anns, res = [], []
    for k in range(D):
        cy, cx, ry, rx, vy, vx = objs[k]
        if k < G:
            m = paint(cy, cx, ry, rx, vy, vx, k)
            anns.append({"id": k + 1, "video_id": 1, "category_id": 1 + k % 2, "iscrowd": 0, "segmentations": R.rle_encode_masks(m),
                         "areas": [int(a) for a in m.sum(dim=(1, 2)).tolist()]})
        m = paint(cy + 0.004 * H, cx - 0.003 * W, ry * 1.03, rx * 0.98, vy, vx, k)
        res.append({"video_id": 1, "score": float(rng.uniform(0.05, 0.99)), "category_id": 1 + k % 2, "segmentations": R.rle_encode_masks(m),
                    "height": H, "width": W})
    gt = {"videos": [{"id": 1, "height": H, "width": W, "length": T}], "categories": [{"id": 1, "name": "a"}, {"id": 2, "name": "b"}],
          "annotations": anns}
    return gt, res


def numpy_reference(d_segs, g_segs):
    """`iou_seq` of one pair as the reference computes it: per frame both masks decoded, intersection and union summed."""
    i = u = 0.0
    for d, g in zip(d_segs, g_segs):
        a, b = R.rle_decode(d).astype(bool), R.rle_decode(g).astype(bool)
        i += float((a & b).sum())
        u += float((a | b).sum())
    return i / u if u > 0 else 0.0


def main():
    ap = bench.arg_parser(reps=10)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ref_pairs", type=int, default=3)
    args = ap.parse_args()
    dev = bench.gpu_or_exit("vis_eval_bench")
    T, H, W, D, G = (6, 120, 214, 12, 3) if args.quick else (36, 720, 1280, 100, 10)
    gt, res = scene(T, H, W, D, G, dev)
    d_runs = vc.runs_from_rles([m for r in res for m in r["segmentations"]], H, W, device=dev)
    g_runs = vc.runs_from_rles([m for a in gt["annotations"] for m in a["segmentations"]], H, W, device=dev)
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "reps": args.reps, "frames": T, "size": [H, W], "detections": D,
           "ground_truths": G, "dt_boundaries": int(d_runs.starts[-1]), "gt_boundaries_max": int(g_runs.starts.diff().max())}
    bench.kernel_vs_aten(out, args, lambda: (vc.vis_video_overlap(d_runs, g_runs, T, H, W),), lambda: (vc.vis_overlap_aten(d_runs, g_runs, T, H, W),),
                         "counts_equal")
    torch.cuda.empty_cache()
    ev, e = bench.timed(lambda: ytvis.evaluate_predictions_on_ytvis(gt, res, device=dev), args.warmup, args.samples)
    n = min(G, args.ref_pairs)
    ref, ious = bench.timed(lambda: [numpy_reference(res[k]["segmentations"], gt["annotations"][k]["segmentations"]) for k in range(n)], 0, 2)
    table = e._video_ious(1)                                           # [detections, ground truths]; pair k is (k, k)
    out["ious_equal"] = bool(all(table[k, k] == ious[k] for k in range(n)))
    out["evaluate_s"] = bench.stats(ev, 3)
    out["evaluate_s_per_pair"] = bench.stats([v / (D * G) for v in ev], 6)
    out["numpy_reference_pairs"] = n
    out["numpy_reference_s_per_pair"] = bench.stats([v / n for v in ref], 5)
    out["evaluate_faster_beyond_spread"] = out["evaluate_s_per_pair"]["max"] < out["numpy_reference_s_per_pair"]["min"]
    out["stats"] = [round(float(s), 6) for s in e.stats]
    print(json.dumps({k: out[k] for k in ("kernel_us", "aten_us", "counts_equal")}), file=sys.stderr, flush=True)
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
