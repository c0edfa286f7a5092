"""Overlay JPEGs of one 20-frame video with 10 objects two ways, at 720 x 1280 and 1080 x 1920 (120 x 214 with --quick), quality 90, 4:2:0;
synthetic structured content from a seed (tools/jpeg_bench.scene) and discs as the objects' id maps.  Prints one JSON line and writes it
to --out.

  launches_ms / coefficients_ms / stream_ms    the launches of csrc/jpeg_encode.hip alone on buffers already on the device: all five, the
                       three of phase 1 (blocks with the fused overlay, sizes, scan) and the two of phase 2 (pack, stuff)
  encode_jpegs_ms      `jpegenc_ops.encode_jpegs` with ids and lut on frames and id maps on the device: the launches, the download of the
                       totals, the allocation of the stream buffers, the download of the streams, headers
  write_gpu_ms / write_host_ms    `results.write_overlay_jpegs` into a temporary folder with jpeg="gpu" (frames and id maps on the device)
                       and with jpeg="host" (numpy overlay + Pillow on host arrays): what a run pays per video
  scratch_bytes / stream_bytes    device bytes beside the inputs; the bytes of the 20 entropy-coded streams
  files_equal          the two writers give the same files

Every group is `--samples` alternating samples after `--warmup` untimed ones: median, min and max.  `gpu_faster_beyond_spread` is
max(write_gpu) < min(write_host): a ratio is claimed only where it holds.

    python tools/overlay_bench.py [--quick] [--samples 5] [--warmup 2] [--out profiles/jpeg_encode_bench_v1.json]
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eval_bench_common as bench                         # noqa: E402
from jpeg_bench import T, alternate, scene                # noqa: E402
from univs_amd import jpegenc_ops                         # noqa: E402
from univs_amd.inference import overlay_rule              # noqa: E402
from univs_amd.inference.results import write_overlay_jpegs   # noqa: E402

OBJECTS = 10


def idmaps(H, W, seed=1):
    """int32 [T, H, W]: OBJECTS discs that move from frame to frame, later ones over earlier ones; 0 elsewhere."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    discs = [(rng.uniform(0.2, 0.8) * H, rng.uniform(0.2, 0.8) * W, rng.uniform(0.05, 0.18) * H, rng.uniform(-5, 5, 2)) for _ in range(OBJECTS)]
    out = np.zeros((T, H, W), np.int32)
    for t in range(T):
        for k, (cy, cx, r, v) in enumerate(discs, 1):
            out[t][(y - cy - t * v[0]) ** 2 + (x - cx - t * v[1]) ** 2 < r * r] = k
    return out


def one(H, W, args, dev):
    frames, ids = scene(H, W), idmaps(H, W)
    lut = overlay_rule.lut_from_palette(overlay_rule.default_palette(OBJECTS + 1))
    rgb_d, ids_d = torch.from_numpy(frames).to(dev), torch.from_numpy(ids).to(dev)
    host_frames = list(frames)
    names = ["/bench/video/%05d.jpg" % i for i in range(T)]
    out = {"frames": T, "size": [H, W], "objects": OBJECTS, "quality": 90, "sampling": "420"}
    launches = []
    res = jpegenc_ops.encode_covered(rgb_d, 90, "420", ids=ids_d, lut=lut, launches=launches)
    assert res is not None and res.status.tolist() == [0] * T, None if res is None else res.status
    out["scratch_bytes"], out["stream_bytes"], out["frame_bytes"] = int(res.scratch_bytes), int(res.stream_bytes), int(rgb_d.numel())
    with tempfile.TemporaryDirectory() as root:
        sides = {"launches": lambda: launches[0](3), "coefficients": lambda: launches[0](1), "stream": lambda: launches[0](2),
                 "encode_jpegs": lambda: jpegenc_ops.encode_jpegs(rgb_d, 90, "420", ids=ids_d, lut=lut),
                 "write_gpu": lambda: write_overlay_jpegs(os.path.join(root, "gpu"), names, 0, rgb_d, ids_d, lut, jpeg="gpu"),
                 "write_host": lambda: write_overlay_jpegs(os.path.join(root, "host"), names, 0, host_frames, ids, lut, jpeg="host")}
        s = alternate(sides, args.warmup, args.samples)
        a, b = sides["write_gpu"](), sides["write_host"]()
        out["files_equal"] = bool(len(a) == len(b) == T and all(open(p, "rb").read() == open(q, "rb").read() for p, q in zip(a, b)))
    for k in sides:
        out[k + "_ms"] = bench.stats([v * 1e3 for v in s[k]], 3)
    out["gpu_faster_beyond_spread"] = out["write_gpu_ms"]["max"] < out["write_host_ms"]["min"]
    out["gpu_slower_beyond_spread"] = out["write_gpu_ms"]["min"] > out["write_host_ms"]["max"]
    return out


def main():
    ap = bench.arg_parser(reps=1)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = bench.gpu_or_exit("overlay_bench")
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "cases": []}
    for H, W in ([(120, 214)] if args.quick else [(720, 1280), (1080, 1920)]):
        out["cases"].append(one(H, W, args, dev))
        print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
