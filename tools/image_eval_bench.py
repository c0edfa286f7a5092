"""Times the image chain's two kernels and its two evaluators on one MI355X, at the shapes of the shipped image configs:

    COCO     C = 133, r 800 x 1066 -> 480 x 640
    ADE20K   C = 150, r 512 x 683  -> 512 x 683 (identity) and -> 1024 x 1366

Per geometry: `imagelabels_ops.semseg_labels(r, size)` against the dense formulation on the parent's kernels in the same run,
`ops.bilinear_resample(r, size).argmax(0)` (alternating samples, min / max reported; the results compared byte for byte); the
allocator's peak above the inputs and the result on both sides; `label_confusion_u8` against `label_confusion_aten` on two label maps of
the output size; and `SemSegEvaluator.process` / `PanopticEvaluator.process` per image (ground-truth PNGs on disk, png and reader
"host" and "gpu").  The bytes each side of the labels comparison moves are computed from the shapes and printed beside the times.

    python tools/image_eval_bench.py [--samples 5] [--warmup 2] [--reps 5] [--out profiles/image_eval_bench_v1.json]

No GPU: it fails.  A ratio is stated only where the two min-max ranges do not overlap (`kernel_faster_beyond_spread`).
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_bench_common as common  # noqa: E402
from univs_amd import imagelabels_ops as il  # noqa: E402
from univs_amd import ops  # noqa: E402
from univs_amd.evaluation import image as ie  # noqa: E402

CASES = [("coco_800x1066_to_480x640", 133, (800, 1066), (480, 640)), ("ade20k_512x683_identity", 150, (512, 683), (512, 683)),
         ("ade20k_512x683_to_1024x1366", 150, (512, 683), (1024, 1366))]


def scores(C, hw, seed):
    """float32 [C, h, w] on the device: smooth per-class fields plus noise, so that regions of one label and their borders both occur."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.randn((1, C, max(2, hw[0] // 64), max(2, hw[1] // 64)), generator=g, device="cuda")
    smooth = torch.nn.functional.interpolate(coarse, size=hw, mode="bilinear", align_corners=False)[0]
    return (smooth + 0.05 * torch.randn((C,) + tuple(hw), generator=g, device="cuda")).contiguous()


def peak_above(fn, keep):
    """The allocator's peak during fn() above what was allocated before it plus the result's own bytes."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return int(peak - keep(r))


def bench_case(args, dev, folder, name, C, in_hw, out_hw):
    r = scores(C, in_hw, len(name))
    H, W = out_hw

    def kernel():
        return (il.semseg_labels(r, out_hw),)

    def dense():
        return (ops.bilinear_resample(r, out_hw).argmax(0).to(torch.uint8),)

    out = {"classes": C, "in_hw": list(in_hw), "out_hw": list(out_hw)}
    lab = {}
    common.kernel_vs_aten(lab, args, kernel, dense, "labels_equal")
    # bytes from the shapes: both sides read r once (a down-scale's taps still touch every cache line); the dense side also writes the
    # [C, H, W] tensor and reads it back, and writes int64 labels and their uint8 copy
    r_bytes, dense_tensor = C * in_hw[0] * in_hw[1] * 4, C * H * W * 4
    lab["kernel_bytes"] = r_bytes + H * W
    lab["dense_bytes"] = r_bytes + 2 * dense_tensor + H * W * (8 + 8 + 1)
    lab["kernel_GBps"] = round(lab["kernel_bytes"] / (lab["kernel_us"]["median"] * 1e-6) / 1e9, 1)
    lab["dense_GBps"] = round(lab["dense_bytes"] / (lab["aten_us"]["median"] * 1e-6) / 1e9, 1)
    lab["kernel_peak_bytes_above_result"] = peak_above(lambda: kernel()[0], lambda t: t.numel())
    lab["dense_peak_bytes_above_result"] = peak_above(lambda: dense()[0], lambda t: t.numel())
    if lab["kernel_faster_beyond_spread"]:
        lab["dense_over_kernel"] = round(lab["aten_us"]["median"] / lab["kernel_us"]["median"], 2)
    out["labels"] = lab

    pred = kernel()[0]
    gt = pred.clone()
    flip = torch.rand(pred.shape, device=dev) < 0.2
    gt[flip] = torch.randint(0, C, (int(flip.sum()),), device=dev, dtype=torch.uint8)
    gt[torch.rand(pred.shape, device=dev) < 0.05] = 255

    def conf_kernel():
        c, s = il.new_confusion(C, dev)
        assert il.label_confusion_u8(gt, pred, C, 255, c, s)
        return c, s

    def conf_aten():
        c, s = il.new_confusion(C, dev)
        il.label_confusion_aten(gt, pred, C, 255, c, s)
        return c, s

    conf = {}
    common.kernel_vs_aten(conf, args, conf_kernel, conf_aten, "counts_equal", algorithmic_bytes=2 * H * W)
    conf["kernel_peak_bytes_above_result"] = peak_above(conf_kernel, lambda t: sum(x.numel() * 8 for x in t))
    conf["aten_peak_bytes_above_result"] = peak_above(conf_aten, lambda t: sum(x.numel() * 8 for x in t))
    if conf["kernel_faster_beyond_spread"]:
        conf["aten_over_kernel"] = round(conf["aten_us"]["median"] / conf["kernel_us"]["median"], 2)
    out["confusion"] = conf

    # the evaluators' process() per image, ground truth on disk
    from PIL import Image
    sub = os.path.join(folder, name)
    os.makedirs(sub)
    Image.fromarray(gt.cpu().numpy()).save(os.path.join(sub, "im.png"))
    item = {"file_names": ["/x/im.jpg"], "file_name": "/x/im.jpg", "image_id": "im"}
    block = 128                                                      # a panoptic map of square segments, ids 1 .. n, class = id % C
    ys, xs = torch.arange(H, device=dev) // block, torch.arange(W, device=dev) // block
    pan = (ys[:, None] * ((W + block - 1) // block) + xs[None, :] + 1).to(torch.int32)
    n_seg = int(pan.max())
    cats = [{"id": c + 1, "name": str(c), "isthing": int(c % 2)} for c in range(C)]
    pan_np = pan.cpu().numpy().astype(np.int64)
    Image.fromarray(np.stack([pan_np % 256, pan_np // 256 % 256, pan_np // 65536], -1).astype(np.uint8)).save(os.path.join(sub, "pan.png"))
    with open(os.path.join(sub, "gt.json"), "w") as f:
        json.dump({"categories": cats, "annotations": [{"image_id": "im", "file_name": "pan.png", "segments_info": [
            {"id": k, "category_id": k % C + 1, "iscrowd": 0, "area": int((pan_np == k).sum())} for k in range(1, n_seg + 1)]}]}, f)
    infos = [{"id": k, "isthing": bool((k % C) % 2), "category_id": k % C} for k in range(1, n_seg + 1)]
    out["segments"] = n_seg
    for mode in ("host", "gpu"):
        sem = ie.SemSegEvaluator(sub, C, 255, None, None, device=dev, reader=mode)
        pq = ie.PanopticEvaluator(os.path.join(sub, "gt.json"), sub, os.path.join(sub, "out_" + mode), device=dev, png=mode, reader=mode)

        def sem_process():
            sem.process([item], [{"sem_seg_labels": pred}])
            torch.cuda.synchronize()

        def pq_process():
            pq.process([item], [{"panoptic_seg": (pan, infos)}])
            torch.cuda.synchronize()
        s, _ = common.timed(sem_process, args.warmup, args.samples)
        out[f"semseg_process_{mode}_ms"] = common.stats([1e3 * v for v in s])
        s, _ = common.timed(pq_process, args.warmup, args.samples)
        out[f"panoptic_process_{mode}_ms"] = common.stats([1e3 * v for v in s])
        out[f"panoptic_pq_{mode}"] = pq.evaluate()["panoptic_seg"]["PQ"]
    return out


def main():
    args = common.arg_parser(reps=5).parse_args()
    dev = common.gpu_or_exit("image_eval_bench")
    out = {"tool": "image_eval_bench", "device": torch.cuda.get_device_name(0), "samples": args.samples, "warmup": args.warmup,
           "kernel_reps": args.reps, "cases": {}}
    with tempfile.TemporaryDirectory() as folder:
        for name, C, in_hw, out_hw in CASES:
            out["cases"][name] = bench_case(args, dev, folder, name, C, in_hw, out_hw)
    common.emit(out, args.out)


if __name__ == "__main__":
    main()
