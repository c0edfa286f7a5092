"""Scoring one synthetic 720p video (20 frames, about 40 segments on each side) three ways.  Prints one JSON line
and writes it to --out:

  kernel_us / aten_us      the pair tables of the video (uint8 RGB on both sides, already on the device) from csrc/pair_count.hip and from
                           `pair_counts_aten` on the same GPU: median, min and max over `--samples` samples after `--warmup` untimed ones,
                           alternating, the id tables on the device too; a sample is the synchronised wall time of `--reps` back-to-back kernel calls (one ATen call)
  kernel_GBps              the algorithmic bytes (6 B per pixel: both RGB maps read once) over the median kernel time
  big_table                the same two timings for the same frames under 127 segments on each side: (127 + 1)^2 = 16384 cells, the
                           largest histogram the kernel covers
  evaluate_files_s         the whole `evaluate_vps_files` on the video's tree: every PNG decoded once, one upload, one table, the metrics
  numpy_pixel_passes_s     the pixel passes of the reference's algorithm restated in numpy on the same host: for every window of 1, 2, 4, 6
                           and 8 frames the PNGs of the window decoded again, `np.unique` of each predicted frame and of the window's 64-bit
                           pair keys and one count per ground-truth id (eval_vpq_vps.py:83-165); then per frame the two label maps painted
                           with one `==` pass per segment and STQuality's `np.unique` calls (eval_stq_vps.py:134-161).  The matching
                           itself, which costs little, is left out: a lower bound of the reference's time.

    python tools/vps_eval_bench.py [--samples 5] [--warmup 2] [--reps 20] [--kernel-only] [--out FILE]
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eval_bench_common as bench                       # noqa: E402
from univs_amd.evaluation import pair_counts as pc      # noqa: E402
from univs_amd.evaluation import vps                    # noqa: E402

T, H, W, SEGS, BIG_SEGS = 20, 720, 1280, 40, 126      # (VOID joins each table: 41 and 127 ids)


def scene(seed=0, SEGS=SEGS):
    """Stuff bands under moving rectangles; the prediction is the ground truth shifted by a few pixels, under other ids."""
    rng = np.random.default_rng(seed)
    ids = {"gt": [int(r) + 256 * int(g) + 65536 * int(b) for r, g, b in rng.integers(1, 256, (SEGS, 3))],
           "pred": [int(r) + 256 * int(g) + 65536 * int(b) for r, g, b in rng.integers(1, 256, (SEGS, 3))]}
    boxes = [(int(rng.integers(0, H - 120)), int(rng.integers(0, W - 200)), int(rng.integers(40, 120)), int(rng.integers(60, 200)),
              int(rng.integers(-3, 4)), int(rng.integers(-5, 6))) for _ in range(SEGS - 6)]
    maps = {}
    for side, off in (("gt", 0), ("pred", 3)):
        pan = np.zeros((T, H, W), np.int32)
        for t in range(T):
            for k in range(6):
                pan[t, k * 120 + (off if k else 0):(k + 1) * 120 + off] = ids[side][k]
            for k, (y, x, h, w, dy, dx) in enumerate(boxes):
                y0, x0 = max(0, y + dy * t + off), max(0, x + dx * t + off)
                pan[t, y0:y0 + h, x0:x0 + w] = ids[side][6 + k]
        maps[side] = pan
    cats = [{"id": c, "isthing": int(c >= 6), "color": [c, c, c]} for c in range(SEGS)]

    def frames(side):
        return [{"file_name": "%08d.png" % t, "segments_info": [
            {"id": i, "category_id": k, "iscrowd": 0, "area": int((maps[side][t] == i).sum())} for k, i in enumerate(ids[side]) if (maps[side][t] == i).any()]}
            for t in range(T)]
    gt_json = {"categories": cats, "videos": [{"video_id": "v", "images": [{"file_name": "%08d.png" % t} for t in range(T)]}],
               "annotations": [{"video_id": "v", "annotations": frames("gt")}]}
    pred_json = {"annotations": [{"video_id": "v", "annotations": frames("pred")}]}
    return maps, gt_json, pred_json


def rgb(ids):
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


def write_tree(root, maps, gt_json, pred_json):
    from PIL import Image
    for sub, side in ((os.path.join(root, "truth", "v"), "gt"), (os.path.join(root, "submit", "pan_pred", "v"), "pred")):
        os.makedirs(sub, exist_ok=True)
        for t in range(T):
            Image.fromarray(rgb(maps[side][t])).save(os.path.join(sub, "%08d.png" % t))
    with open(os.path.join(root, "submit", "pred.json"), "w") as f:
        json.dump(pred_json, f)
    with open(os.path.join(root, "gt.json"), "w") as f:
        json.dump(gt_json, f)
    return os.path.join(root, "submit"), os.path.join(root, "truth"), os.path.join(root, "gt.json")


def numpy_pixel_passes(submit, truth, gt_json, pred_json):
    from PIL import Image

    def ids_of(path):
        a = np.uint32(np.array(Image.open(path)))
        return a[:, :, 0] + a[:, :, 1] * 256 + a[:, :, 2] * 256 * 256
    names = [im["file_name"] for im in gt_json["videos"][0]["images"]]
    gt_fr, pred_fr = gt_json["annotations"][0]["annotations"], pred_json["annotations"][0]["annotations"]
    for nframes in vps.NFRAMES:
        for idx in range(len(names) - nframes + 1):
            gts, preds = [], []
            for n in names[idx:idx + nframes]:
                gts.append(ids_of(os.path.join(truth, "v", n)))
                preds.append(ids_of(os.path.join(submit, "pan_pred", "v", n)))
                np.unique(preds[-1], return_counts=True)
            g, p = np.stack(gts), np.stack(preds)
            labels, _ = np.unique(g.astype(np.uint64) * (256 ** 3) + p.astype(np.uint64), return_counts=True)
            for gid in np.unique(labels // (256 ** 3)):
                np.sum(g == gid)
    for t, n in enumerate(names):
        g, p = ids_of(os.path.join(truth, "v", n)), ids_of(os.path.join(submit, "pan_pred", "v", n))
        painted = []
        for pan, fr in ((g, gt_fr[t]), (p, pred_fr[t])):
            sem, ins = np.ones_like(pan) * 255, np.ones_like(pan) * 255
            for k, el in enumerate(fr["segments_info"]):
                sem[pan == el["id"]] = el["category_id"]
                ins[pan == el["id"]] = k
            painted.append(((sem << 16) + ins).astype(np.int64))
        yt, yp = painted
        np.unique(((yt >> 16) << 16) + (yp >> 16), return_counts=True)
        mask = (yt >> 16) >= 6
        np.unique(yp[mask], return_counts=True)
        np.unique(yt[mask], return_counts=True)
        np.unique(yt[mask] * 2 ** 24 + yp[mask], return_counts=True)


def main():
    ap = bench.arg_parser(reps=20)
    ap.add_argument("--kernel-only", action="store_true", help="skip the ATen and the host sides (the run under the kernel trace)")
    args = ap.parse_args()
    dev = bench.gpu_or_exit("vps_eval_bench")
    maps, gt_json, pred_json = scene()
    gt_ids = torch.from_numpy(vps.id_table(gt_json["annotations"][0]["annotations"])).to(dev)
    pred_ids = torch.from_numpy(vps.id_table(pred_json["annotations"][0]["annotations"])).to(dev)
    g, p = torch.from_numpy(rgb(maps["gt"])).to(dev), torch.from_numpy(rgb(maps["pred"])).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "frames": T, "size": [H, W], "ids": [int(gt_ids.numel()), int(pred_ids.numel())],
           "samples": args.samples, "reps": args.reps}

    def table_times(g, p, gt_ids, pred_ids, out):
        bench.kernel_vs_aten(out, args, lambda: pc.panoptic_pair_counts(g, p, gt_ids, pred_ids),
                             None if args.kernel_only else lambda: pc.pair_counts_aten(g, p, gt_ids, pred_ids, with_unknown=True),
                             "tables_equal", 6 * T * H * W)
    out["algorithmic_bytes"] = 6 * T * H * W
    table_times(g, p, gt_ids, pred_ids, out)
    big_maps, big_gt, big_pred = scene(1, BIG_SEGS)
    big_ids = [torch.from_numpy(vps.id_table(j["annotations"][0]["annotations"])).to(dev) for j in (big_gt, big_pred)]
    out["big_table"] = {"ids": [int(v.numel()) for v in big_ids]}
    table_times(torch.from_numpy(rgb(big_maps["gt"])).to(dev), torch.from_numpy(rgb(big_maps["pred"])).to(dev), *big_ids, out["big_table"])
    if not args.kernel_only:
        with tempfile.TemporaryDirectory() as root:
            submit, truth, gt_file = write_tree(root, maps, gt_json, pred_json)
            ev, _ = bench.timed(lambda: vps.evaluate_vps_files(submit, truth, gt_file, device=dev, output_dir=os.path.join(root, "scores")),
                                args.warmup, args.samples)
            ref, _ = bench.timed(lambda: numpy_pixel_passes(submit, truth, gt_json, pred_json), 0, 2)
        out["evaluate_files_s"] = bench.stats(ev, 3)
        out["numpy_pixel_passes_s"] = bench.stats(ref, 3)
        out["evaluate_faster_beyond_spread"] = out["evaluate_files_s"]["max"] < out["numpy_pixel_passes_s"]["min"]
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
