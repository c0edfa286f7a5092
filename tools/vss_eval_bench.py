"""Scoring one synthetic VSPW-shaped video (480 x 853, 60 frames, 124 classes; 120 x 213, 20 frames with --quick) four ways.  Prints
one JSON line and writes it to --out:

  kernel_us / aten_us      the counts of the video (both uint8 stacks already on the device) from csrc/vss_count.hip and from
                           `vss_counts_aten` on the same GPU: median, min and max over `--samples` samples after `--warmup` untimed
                           ones, alternating; a sample is the synchronised wall time of `--reps` back-to-back kernel calls (one ATen
                           call), the output allocations of the wrapper included
  kernel_GBps              the algorithmic bytes (2 B per pixel and frame: both maps read once) over the median kernel time
  evaluate_files_s         the whole `evaluate_vss_files` on the video's tree: every PNG decoded once, one upload, one launch, the scores
  numpy_reference_s        the reference's algorithm restated in numpy on the same host from its description: per file the mapped ground
                           truth and one bincount of the flattened cells; then for each clip length every file decoded again and, for
                           every window start, frame i compared with each of the next n - 1 frames on both sides (on stacked uint8
                           frames with boolean planes, where the reference keeps float64 planes: a lower bound of its time)

    python tools/vss_eval_bench.py [--quick] [--samples 5] [--warmup 2] [--reps 20] [--out profiles/vss_eval_bench_v1.json]
"""
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eval_bench_common as bench                       # noqa: E402
from univs_amd.evaluation import vss                    # noqa: E402
from univs_amd.evaluation import vss_counts as vc       # noqa: E402

C = 124


def scene(T, H, W, seed=0):
    """Raw gt: horizontal bands under moving rectangles, a void border; prediction: the classes shifted by a few pixels, a patch that
    flickers and 1 % single-pixel noise."""
    rng = np.random.default_rng(seed)
    boxes = [(int(rng.integers(0, H - H // 4)), int(rng.integers(0, W - W // 4)), int(rng.integers(H // 12, H // 4)),
              int(rng.integers(W // 12, W // 4)), int(rng.integers(-2, 3)), int(rng.integers(-3, 4)), int(rng.integers(10, 125))) for _ in range(30)]
    maps = []
    for off in (0, 2):
        m = np.zeros((T, H, W), np.uint8)
        for t in range(T):
            for k in range(6):
                m[t, k * H // 6 + (off if k else 0):] = 1 + k
            for y, x, h, w, dy, dx, c in boxes:
                y0, x0 = max(0, y + dy * t + off), max(0, x + dx * t + off)
                m[t, y0:y0 + h, x0:x0 + w] = c
        maps.append(m)
    gt, pred = maps
    gt[:, :, :4] = 255
    gt[:, :3, :] = 0
    pred = pred - 1
    for t in range(T):
        if t % 4 == 0:
            pred[t, H // 2:H // 2 + H // 10, W // 2:W // 2 + W // 10] = 77
        flip = rng.random((H, W)) < 0.01
        pred[t][flip] = rng.integers(0, C, int(flip.sum()))
    return gt, pred


def write_tree(root, gt, pred):
    from PIL import Image
    data, submit = os.path.join(root, "VSPW"), os.path.join(root, "submit")
    for sub, m in ((os.path.join(data, "data", "v", "mask"), gt), (os.path.join(submit, "v"), pred)):
        os.makedirs(sub, exist_ok=True)
        for t in range(len(m)):
            Image.fromarray(m[t]).save(os.path.join(sub, "%08d.png" % t))
    with open(os.path.join(data, "val.txt"), "w") as f:
        f.write("v\n")
    return submit, data


def numpy_reference(submit, data):
    from PIL import Image

    table = ((np.arange(256) - 1) % 256).astype(np.uint8)             # raw -> label: 0 -> 255, v -> v - 1 ...
    table[255] = 255                                                  # ... and void stays void

    def mapped(path):
        return table[np.array(Image.open(path))]
    mask_dir = os.path.join(data, "data", "v", "mask")
    confusion = np.zeros((C, C))
    for name in os.listdir(mask_dir):
        g, p = mapped(os.path.join(mask_dir, name)), np.array(Image.open(os.path.join(submit, "v", name)))
        keep = g < C
        confusion += np.bincount(C * g[keep].astype(int) + p[keep], minlength=C * C).reshape(C, C)
    scores = [confusion]
    for n in (8, 16):                                                 # every file decoded again per clip length, as the reference
        names = sorted(os.listdir(mask_dir))
        gs = np.stack([mapped(os.path.join(mask_dir, name)) for name in names])
        ps = np.stack([np.array(Image.open(os.path.join(submit, "v", name))) for name in names])
        ratios = []
        for i in range(len(names) - n):                               # frame i against the n - 1 frames behind it, per window
            keeps_g = (gs[i + 1:i + n] == gs[i]).all(axis=0)
            keeps_p = (ps[i + 1:i + n] == ps[i]).all(axis=0)
            den = np.count_nonzero(keeps_g)
            ratios.append(np.count_nonzero(keeps_g & keeps_p) / den if den else np.nan)
        scores.append(np.nanmean(np.array(ratios)))
    return scores


def main():
    ap = bench.arg_parser(reps=20)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = bench.gpu_or_exit("vss_eval_bench")
    T, H, W = (20, 120, 213) if args.quick else (60, 480, 853)
    gt, pred = scene(T, H, W)
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "frames": T, "size": [H, W], "num_classes": C, "samples": args.samples, "reps": args.reps,
           "algorithmic_bytes": 2 * T * H * W}
    bench.kernel_vs_aten(out, args, lambda: vc.vss_video_counts(g, p, C), lambda: vc.vss_counts_aten(g, p, C), "counts_equal", 2 * T * H * W)
    with tempfile.TemporaryDirectory() as root:
        submit, data = write_tree(root, gt, pred)
        ev, score = bench.timed(lambda: vss.evaluate_vss_files(submit, data, "val.txt", C, dev, output_dir=os.path.join(root, "scores")),
                                args.warmup, args.samples)
        ref, theirs = bench.timed(lambda: numpy_reference(submit, data), 0, 2)
    out["scores_equal"] = bool(np.array_equal(theirs[0], score["confusion"]) and theirs[1] == score["VC8"] and theirs[2] == score["VC16"])
    out["evaluate_files_s"] = bench.stats(ev, 3)
    out["numpy_reference_s"] = bench.stats(ref, 3)
    out["evaluate_faster_beyond_spread"] = out["evaluate_files_s"]["max"] < out["numpy_reference_s"]["min"]
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
