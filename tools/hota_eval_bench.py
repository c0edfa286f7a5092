"""HOTA of one synthetic YouTube-VIS-shaped video four ways: the `vis_eval_bench.py` case, 36 frames at 720 x 1280 with 100 tracks and 10
ground truths in two categories (6 frames at 120 x 214 with 12 and 3 with --quick).  Prints one JSON line and writes it to --out.

  kernel_us / aten_us   the HOTA tables of the video (overlap table and areas already on the device) from csrc/hota_count.hip and from
                        `hota_counts_aten` (the rule in numpy on the host, one scipy assignment per frame, download and upload
                        included) on the same tensors: median, min and max over `--samples` samples after `--warmup` untimed ones,
                        alternating; a kernel sample is the synchronised wall time of `--reps` back-to-back wrapper calls (uploads of the
                        id lists and output allocations included), an ATen sample one call
  evaluate_s            `evaluate_hota_files` end to end on the annotation and result records: strings decoded to runs, the overlap
                        launch, the HOTA launch, the host-side fields and combinations
  host_loop_s           the reference's frame loops alone (`hota_counts.sequence_counts`: numpy and one scipy call per frame) on host
                        arrays that already hold the similarities, both classes: what the kernel replaces, without any transfer

No speed was promised for this kernel; `kernel_faster_beyond_spread` is max(kernel) < min(aten), `kernel_faster_than_host_loop` the
same against the host loop.

    python tools/hota_eval_bench.py [--quick] [--samples 5] [--warmup 2] [--reps 10] [--out profiles/hota_eval_bench_v1.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_bench_common as bench                         # noqa: E402
from vis_eval_bench import scene                          # noqa: E402
from univs_amd.evaluation import hota                     # noqa: E402
from univs_amd.evaluation import hota_counts as hc        # noqa: E402


def main():
    ap = bench.arg_parser(reps=10)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = bench.gpu_or_exit("hota_eval_bench")
    T, H, W, D, G = (6, 120, 214, 12, 3) if args.quick else (36, 720, 1280, 100, 10)
    gt, res = scene(T, H, W, D, G, dev)
    calls = []
    real = hota.hota_counts
    hota.hota_counts = lambda *a: calls.append(a) or real(*a)
    try:
        first = hota.evaluate_hota_files(gt, res, device=dev)
    finally:
        hota.hota_counts = real
    (call,) = calls
    gt_area, tr_area, inter, gt_ids, gt_starts, tr_ids, tr_starts, thr = call
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "reps": args.reps, "frames": T, "size": [H, W], "tracks": D,
           "ground_truths": G, "classes": len(gt_starts) - 1, "ids_per_class": [np.diff(gt_starts).tolist(), np.diff(tr_starts).tolist()]}
    bench.kernel_vs_aten(out, args, lambda: tuple(hc.hota_video_counts(*call)), lambda: tuple(hc.hota_counts_aten(*call)), "tables_equal")
    ev, last = bench.timed(lambda: hota.evaluate_hota_files(gt, res, device=dev), args.warmup, args.samples)
    ga, ta, it = gt_area.cpu().numpy(), tr_area.cpu().numpy(), inter.cpu().numpy()
    seqs = []
    for c in range(len(gt_starts) - 1):
        gi, pi = gt_ids[gt_starts[c]:gt_starts[c + 1]], tr_ids[tr_starts[c]:tr_starts[c + 1]]
        seqs.append((hc.similarities(ga[gi], ta[pi], it[np.ix_(pi, gi)]), ga[gi].T > 0, ta[pi].T > 0))
    loop, _ = bench.timed(lambda: [hc.sequence_counts(*s, thr) for s in seqs], args.warmup, args.samples)
    out["evaluate_s"] = bench.stats(ev, 4)
    out["host_loop_s"] = bench.stats(loop, 5)
    out["kernel_faster_than_host_loop"] = out["kernel_us"]["max"] * 1e-6 < out["host_loop_s"]["min"]
    out["results_equal"] = bool(all(np.asarray(first["cls_comb_det_av"][f]).tobytes() == np.asarray(last["cls_comb_det_av"][f]).tobytes()
                                    for f in hota.FIELDS))
    out["summary"] = {k: round(v, 6) for k, v in last["summary"]["cls_comb_det_av"].items()}
    print(json.dumps({k: out[k] for k in ("kernel_us", "aten_us", "tables_equal")}), file=sys.stderr, flush=True)
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
