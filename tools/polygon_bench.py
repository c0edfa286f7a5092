"""Times the polygon rasteriser and the COCO mask-AP scorer on a seeded annotation file shaped like COCO val2017.

    python tools/polygon_bench.py [--images 5000] [--dets 100] [--samples 5] [--eval-images N] [--out profiles/polygon_raster_bench_v1.json]

The file: `--images` images of 480 x 640, about 7 objects each, 1 to 3 polygons of 20 to 60 points.  Timed, `--samples` samples each,
taken in turn (a, b, c, d, a, b, ...) so that a drift of the machine lands on all of them, reported as minimum to maximum:

  launch       the kernel alone (csrc/polygon_runs.hip), the tables already on the device
  device       polygon_ops.polygons_to_runs: host packing and counts, the upload, the launch, the status download, the compaction
  host         polygon_rule.runs_from_polygons_host on the same host
  evaluate     COCOSegmEval end to end (construction, evaluate, accumulate, summarize) with `--dets` detections per image, on the
               first `--eval-images` images (default: all)

and the allocator's peak during `device` above the uploaded tables and the returned `Runs`.  There is no earlier number and no
pycocotools to compare with: the numbers are this project's, no ratio to another implementation is claimed.  One JSON object is
printed and written to `--out`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from univs_amd import polygon_ops  # noqa: E402
from univs_amd.data import polygon_rule as rule  # noqa: E402
from univs_amd.evaluation.coco import evaluate_predictions_on_coco  # noqa: E402

H, W = 480, 640


def blob(rng, cx, cy, r):
    k = int(rng.integers(20, 61))
    t = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * rng.uniform(0.7, 1.0, k)
    return np.round(np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], 1), 2).reshape(-1).tolist()


def annotation_file(images, seed=0):
    rng = np.random.default_rng(seed)
    anns = []
    for i in range(1, images + 1):
        for _ in range(int(rng.integers(1, 14))):
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), float(rng.choice([8, 15, 30, 60, 120])) * rng.uniform(0.7, 1.3)
            polys = [blob(rng, cx + rng.normal(0, 0.5 * r), cy + rng.normal(0, 0.5 * r), r) for _ in range(int(rng.integers(1, 4)))]
            anns.append({"id": len(anns) + 1, "image_id": i, "category_id": int(rng.integers(1, 81)), "segmentation": polys, "iscrowd": 0})
    return {"images": [{"id": i, "height": H, "width": W} for i in range(1, images + 1)], "annotations": anns,
            "categories": [{"id": c, "name": f"c{c}"} for c in range(1, 81)]}


def detections(dataset, per_image, device, seed=1):
    """`per_image` detections per image: the ground truths jittered, then blobs of nothing; masks as uncompressed RLE."""
    rng = np.random.default_rng(seed)
    by_image = {}
    for a in dataset["annotations"]:
        by_image.setdefault(a["image_id"], []).append(a)
    objects, meta = [], []
    for im in dataset["images"]:
        gts = by_image.get(im["id"], [])
        for j in range(per_image):
            if j < len(gts):
                polys = [(np.asarray(p) + rng.normal(0, 1.5, len(p))).round(2).tolist() for p in gts[j]["segmentation"]]
                cat = gts[j]["category_id"]
            else:
                polys = [blob(rng, rng.uniform(0, W), rng.uniform(0, H), rng.uniform(5, 60))]
                cat = int(rng.integers(1, 81))
            objects.append(polys)
            meta.append((im["id"], cat, float(np.round(rng.uniform(0.05, 1.0), 3))))
    runs = polygon_ops.polygons_to_runs_else_host(objects, [(H, W)] * len(objects), device)
    b, s = runs.bounds.cpu().numpy().astype(np.int64), runs.starts.cpu().numpy()
    out = []
    for i, (image_id, cat, score) in enumerate(meta):
        seg = b[s[i]:s[i + 1]]
        out.append({"image_id": image_id, "category_id": cat, "score": score,
                    "segmentation": {"size": [H, W], "counts": np.diff(seg, prepend=0).tolist()}})
    return out


def timed(fn, device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    t = time.perf_counter()
    r = fn()
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    return time.perf_counter() - t, r


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--eval-images", type=int, default=None)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", default=os.path.join("profiles", "polygon_raster_bench_v1.json"))
    args = ap.parse_args(argv)
    device = torch.device(args.device)
    dataset = annotation_file(args.images)
    objects = [a["segmentation"] for a in dataset["annotations"]]
    sizes = [(H, W)] * len(objects)
    plan = polygon_ops.plan(objects, sizes)
    on_device = polygon_ops.upload(plan, device)
    polygon_ops.launch(plan, on_device)                                   # warm-up: the code object, the LDS attribute
    want = rule.runs_from_polygons_host(objects[:2000], sizes[:2000])
    got = polygon_ops.polygons_to_runs(objects[:2000], sizes[:2000], device)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want)), "the kernel and the host formulation disagree"
    # areas for the ground truth (COCO's json carries them), from the rasteriser itself
    areas = polygon_ops.polygons_to_runs(objects, sizes, device).areas().cpu().tolist()
    status = polygon_ops.LAST_STATUS
    for a, area in zip(dataset["annotations"], areas):
        a["area"] = area
    n_eval = args.eval_images or args.images
    sub = {"images": dataset["images"][:n_eval], "categories": dataset["categories"],
           "annotations": [a for a in dataset["annotations"] if a["image_id"] <= n_eval]}
    dets = detections(sub, args.dets, device)
    samples = {"launch": [], "device": [], "host": [], "evaluate": []}
    peak = 0
    for _ in range(args.samples):
        samples["launch"].append(timed(lambda: polygon_ops.launch(plan, on_device), device)[0])
        torch.cuda.reset_peak_memory_stats(device)
        before = torch.cuda.memory_allocated(device)
        t, runs = timed(lambda: polygon_ops.polygons_to_runs(objects, sizes, device), device)
        samples["device"].append(t)
        kept = plan.blob.nbytes + sum(x.numel() * x.element_size() for x in runs)
        peak = max(peak, torch.cuda.max_memory_allocated(device) - before - kept)
        del runs
        samples["host"].append(timed(lambda: rule.runs_from_polygons_host(objects, sizes), device)[0])
        t, ev = timed(lambda: evaluate_predictions_on_coco(sub, dets, device), device)
        samples["evaluate"].append(t)
    result = {"bench": "polygon_raster", "device": torch.cuda.get_device_name(device) if device.type == "cuda" else "cpu",
              "images": args.images, "image_size": [H, W], "objects": len(objects), "polygons": int(plan.P), "points": int(plan.n_points),
              "vertices": int(plan.n_points), "crossings": int(plan.crossings.sum()), "rasterised_points": int(plan.points_total),
              "objects_left_to_the_host": int((status != 0).sum()), "samples": args.samples,
              "evaluate_images": n_eval, "detections_per_image": args.dets, "AP": float(ev.stats[0]),
              "seconds": {k: {"min": min(v), "max": max(v), "all": v} for k, v in samples.items()},
              "allocator_peak_above_inputs_and_outputs_bytes": int(peak)}
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
