"""Decoding the JPEG frames of one 20-frame video two ways, at 720 x 1280 and 1080 x 1920 (120 x 214 with --quick): 4:2:0 at quality 90,
the common case, and 4:4:4 at quality 95; synthetic structured content from a seed (gradients, moving discs, texture, mild noise),
encoded by Pillow.  Prints one JSON line and writes it to --out.

  host_reader_ms       the parent's path: `read_image` per file on one host core (Pillow on libjpeg-turbo), np.stack, one upload
  decode_jpegs_ms      `jpeg_ops.decode_jpegs` on the same files' bytes in memory: marker walk, one upload of the compressed bytes, the four
                       launches of csrc/jpeg_decode.hip, the status download; decode_jpegs_alone_ms: the same call sampled back to back,
                       not alternating with the other sides
  entropy_ms / pixel_ms / launches_ms   the launches alone on buffers already on the device: the unstuff pre-pass + the parallel Huffman
                       decode, the IDCT + colour conversion, and all four
  rounds               the most synchronisation rounds a chunk took, per file: min / median / max over the files
  mapper_ms            `VideoTestMapper` on the 20 files on disk with decode="host", resize="gpu" (the parent) and decode="gpu"
  scratch_bytes / upload_bytes / decoded_bytes      device scratch of the batch, the bytes uploaded, the decoded frames
  frames_equal / mapper_equal     the two ways give the same bytes

Every group is `--samples` alternating samples after `--warmup` untimed ones: median, min and max.  `*_faster_beyond_spread` is
max(device) < min(host): a ratio is claimed only where it holds.

    python tools/jpeg_bench.py [--quick] [--samples 5] [--warmup 2] [--out profiles/jpeg_decode_bench_v1.json]
"""
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eval_bench_common as bench                         # noqa: E402
from univs_amd import jpeg_ops                            # noqa: E402
from univs_amd.data import VideoTestMapper, read_image    # noqa: E402
from univs_amd.data import jpeg_rule                      # noqa: E402

T = 20
CASES = (("420_q90", 2, 90), ("444_q95", 0, 95))


def scene(H, W, seed=0):
    """uint8 [T, H, W, 3]: a smooth background, textured discs that move from frame to frame, sensor-like noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([110 + 90 * np.sin(x / W * 3.1 + c) * np.cos(y / H * 2.3 - c) for c in range(3)], axis=2)
    texture = 18 * np.sin(x * 0.9) * np.sin(y * 0.7)
    discs = [(rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.04, 0.15) * H, rng.uniform(-6, 6, 2), rng.uniform(0, 255, 3)) for _ in range(12)]
    out = np.empty((T, H, W, 3), np.uint8)
    for t in range(T):
        a = base.copy()
        for cy, cx, r, v, colour in discs:
            m = (y - cy - t * v[0]) ** 2 + (x - cx - t * v[1]) ** 2 < r * r
            a[m] = colour + texture[m][:, None]
        out[t] = np.clip(a + rng.normal(0, 2.5, a.shape), 0, 255).astype(np.uint8)
    return out


def encode(frames, subsampling, quality):
    from PIL import Image
    files = []
    for f in frames:
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, format="JPEG", quality=quality, subsampling=subsampling)
        files.append(buf.getvalue())
    return files


def alternate(sides, warmup, samples):
    """{name: [seconds]} of the host-side functions `sides`, alternating."""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    s = {k: [] for k in sides}
    for _ in range(samples):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            s[k].append(time.perf_counter() - t0)
    return s


def one(H, W, name, subsampling, quality, frames, args, dev):
    files = encode(frames, subsampling, quality)
    out = {"case": name, "frames": T, "size": [H, W], "file_bytes": sum(len(f) for f in files)}
    parsed = [jpeg_rule.parse_jpeg(f) for f in files]
    launches = []
    res = jpeg_ops.decode_covered(parsed, dev, launches=launches)
    assert res.status.tolist() == [0] * T, res.status
    out["rounds"] = {"min": int(res.rounds.min()), "median": float(statistics.median(res.rounds.tolist())), "max": int(res.rounds.max())}
    out["scratch_bytes"], out["upload_bytes"], out["decoded_bytes"] = int(res.scratch_bytes), int(res.upload_bytes), int(res.out.numel())
    with tempfile.TemporaryDirectory() as root:
        paths = []
        for i, f in enumerate(files):
            paths.append(os.path.join(root, "%05d.jpg" % i))
            with open(paths[-1], "wb") as fh:
                fh.write(f)
        record = {"task": "detection", "file_names": paths, "length": T, "height": H, "width": W, "video_id": "bench", "dataset_name": "bench"}
        short, max_size = (min(H, 720), 1280) if not args.quick else (96, 180)
        m_host = VideoTestMapper(short, max_size, resize="gpu", device=dev)
        m_gpu = VideoTestMapper(short, max_size, resize="gpu", device=dev, decode="gpu")

        def host():
            return torch.from_numpy(np.stack([read_image(p) for p in paths])).to(dev)

        def device():
            return jpeg_ops.decode_jpegs(files, dev)[0]
        sides = {"host": host, "device": device, "entropy": lambda: launches[0](1), "pixel": lambda: launches[0](2), "launches": lambda: launches[0](3),
                 "mapper_host": lambda: m_host(record), "mapper_gpu": lambda: m_gpu(record)}
        s = alternate(sides, args.warmup, args.samples)
        s["device_alone"] = alternate({"device": device}, args.warmup, args.samples)["device"]      # back to back, nothing in between
        out["frames_equal"] = bool(torch.equal(host(), device()))
        a, b = m_host(record)["image"], m_gpu(record)["image"]
        out["mapper_equal"] = bool(len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b)))
    for k, key in (("host", "host_reader_ms"), ("device", "decode_jpegs_ms"), ("device_alone", "decode_jpegs_alone_ms"), ("entropy", "entropy_ms"),
                   ("pixel", "pixel_ms"), ("launches", "launches_ms")):
        out[key] = bench.stats([v * 1e3 for v in s[k]], 3)
    out["mapper_ms"] = {"decode_host": bench.stats([v * 1e3 for v in s["mapper_host"]], 3), "decode_gpu": bench.stats([v * 1e3 for v in s["mapper_gpu"]], 3)}
    out["device_faster_beyond_spread"] = out["decode_jpegs_ms"]["max"] < out["host_reader_ms"]["min"]
    out["device_slower_beyond_spread"] = out["decode_jpegs_ms"]["min"] > out["host_reader_ms"]["max"]
    out["mapper_gpu_faster_beyond_spread"] = out["mapper_ms"]["decode_gpu"]["max"] < out["mapper_ms"]["decode_host"]["min"]
    out["mapper_gpu_slower_beyond_spread"] = out["mapper_ms"]["decode_gpu"]["min"] > out["mapper_ms"]["decode_host"]["max"]
    return out


def main():
    ap = bench.arg_parser(reps=1)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cases", default=None, help="comma-separated case names (420_q90, 444_q95)")
    args = ap.parse_args()
    dev = bench.gpu_or_exit("jpeg_bench")
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "subseq_bits": 1024, "cases": []}
    for H, W in ([(120, 214)] if args.quick else [(720, 1280), (1080, 1920)]):
        frames = scene(H, W)
        for name, subsampling, quality in CASES:
            if args.cases and name not in args.cases.split(","):
                continue
            out["cases"].append(one(H, W, name, subsampling, quality, frames, args, dev))
            print(json.dumps(out["cases"][-1]), file=sys.stderr, flush=True)
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
