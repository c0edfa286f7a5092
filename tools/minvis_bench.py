"""Post-processing of the MinVIS-style video drivers at two shipped-like geometries, fused (csrc/video_post.hip) against the ATen
formulation of the same steps (the reference's expressions on the resized [K, V, Hp, Wp] stack).  Prints one JSON line:

  vis_*   InferenceVideoVISFast.postprocess: V = 120 frames of 480 x 854 (480 x 864 padded), mean mask logits [100, 120, 120, 216],
          Q' = K = 100 rows; includes the copy of the bool masks to the host (both paths)
  vps_*   InferenceVideoVPS.postprocess: V = 60 frames of 720 x 1280 (736 x 1280 padded, output 720 x 1280), logits [100, 60, 184, 320],
          40 kept rows
  *_fused_ms / *_aten_ms      median, min and max over `--samples` timed calls after `--warmup` untimed ones (synchronised wall time)
  *_peak_bytes                torch.cuda.max_memory_allocated during one call, above what was allocated before it

The mean mask logits are closed-form moving blobs (masks overlap, enter and leave), the class scores a fixed ramp.

    python tools/minvis_bench.py [--samples 3] [--warmup 1] [--only vis|vps]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from univs_amd.inference.video_minvis import InferenceVideoVISFast, InferenceVideoVPS   # noqa: E402

GEOMETRY = {
    "vis": dict(Q=100, V=120, lowres=(120, 216), padded=(480, 864), crop=(480, 854), out=(480, 854), C=25),
    "vps": dict(Q=100, V=60, lowres=(184, 320), padded=(736, 1280), crop=(720, 1280), out=(720, 1280), C=124, kept=40),
}


def blobs(Q, V, h, w, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, 1, h, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, 1, w)
    t = torch.arange(V, device=dev, dtype=torch.float32).view(1, V, 1, 1)
    r = lambda *s: torch.rand(*s, generator=g, device=dev)
    cy, cx = (r(Q) * h).view(Q, 1, 1, 1), (r(Q) * w).view(Q, 1, 1, 1)
    vy, vx = ((r(Q) - 0.5) * h / V).view(Q, 1, 1, 1), ((r(Q) - 0.5) * w / V).view(Q, 1, 1, 1)
    s = (h / 40 + r(Q) * h / 10).view(Q, 1, 1, 1)
    amp = (4 + 8 * r(Q)).view(Q, 1, 1, 1)
    return -5 + amp * torch.exp(-((yy - cy - vy * t) ** 2 + (xx - cx - vx * t) ** 2) / (2 * s * s))


def timed(fn, warmup, samples):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(samples):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def peak(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def common(g, T=2):
    return dict(num_queries=g["Q"], stability_score_thresh=0.0, size_divisibility=32, LSJ_aug_image_size=1024, LSJ_aug_enable_test=False,
                pixel_mean=[0.0] * 3, pixel_std=[1.0] * 3, num_frames=T, num_frames_window_test=5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", choices=["vis", "vps"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "geometry": GEOMETRY}
    with torch.no_grad():
        for task in ("vis", "vps"):
            if args.only not in (None, task):
                continue
            g = GEOMETRY[task]
            M = blobs(g["Q"], g["V"], *g["lowres"], dev)
            cls = torch.full((g["Q"], g["C"]), 0.01, device=dev)
            cls[torch.arange(g["Q"]), torch.arange(g["Q"]) % g["C"]] = torch.linspace(0.95, 0.2, g["Q"], device=dev)
            if task == "vis":
                mk = lambda fused: InferenceVideoVISFast(test_topk_per_image=100, fused=fused, **common(g)).to(dev)
            else:
                mk = lambda fused: InferenceVideoVPS(test_topk_per_image=g["kept"], object_mask_threshold=0.05, overlap_threshold=0.8,
                                                     thing_dataset_ids=range(1, 59), fused=fused, **common(g)).to(dev)
            res = {}
            for name, fused in (("fused", True), ("aten", False)):
                d = mk(fused)

                def run():
                    res[name] = d.postprocess(cls, M, g["padded"], g["crop"], g["out"])

                out[f"{task}_{name}_ms"] = timed(run, args.warmup, args.samples)
                out[f"{task}_{name}_peak_bytes"] = peak(run)
            out[f"{task}_mean_logits_bytes"] = M.numel() * 4
            out[f"{task}_stack_bytes"] = g["Q"] * g["V"] * g["padded"][0] * g["padded"][1] * 4
            if task == "vis":
                out["vis_records"] = len(res["fused"]["pred_scores"])
                out["vis_labels_equal"] = res["fused"]["pred_labels"] == res["aten"]["pred_labels"]
            else:
                out["vps_segments"] = len(res["fused"]["segments_infos"])
                out["vps_segments_equal"] = res["fused"]["segments_infos"] == res["aten"]["segments_infos"]
                out["vps_map_pixels_differing"] = int((res["fused"]["pred_masks"] != res["aten"]["pred_masks"]).sum())
            out[f"{task}_speedup"] = round(out[f"{task}_aten_ms"]["median"] / out[f"{task}_fused_ms"]["median"], 2)
            del M, res
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
