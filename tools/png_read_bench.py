"""Reading the PNGs of one 20-frame video two ways, at 720 x 1280 and 1080 x 1920 (120 x 214 with --quick): palette id maps with 10
objects and RGB panoptic maps with 30 segments, each written by Pillow at its default level and by png="gpu" (csrc/png_deflate.hip).
Prints one JSON line and writes it to --out.

  host_reader_ms     what the scorers do today: `np.array(PIL.Image.open(path))` per file on one host core, np.stack, one upload
  device_reader_ms   `png_read_ops.read_pngs_device` on the same files' bytes in memory: container parse, one upload of the streams, the two
                     launches of csrc/png_inflate.hip, the status download; uncovered="raise", so nothing passes through Pillow
  launches_ms        the two launches alone, on buffers already on the device
  planes_equal       the two readers' planes are the same bytes
  evaluate_pvos_files_s / evaluate_vps_files_s   the whole scorer on the video's tree with reader="host" and reader="gpu"

Every pair is `--samples` alternating samples after `--warmup` untimed ones: median, min and max.  `device_faster_beyond_spread` is
max(device) < min(host): a ratio is claimed only where it holds.

    python tools/png_read_bench.py [--quick] [--samples 5] [--warmup 2] [--out profiles/png_read_bench_v1.json]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import eval_bench_common as bench                         # noqa: E402
import pvos_eval_bench                                    # noqa: E402
import vps_eval_bench                                     # noqa: E402
from univs_amd import png_ops, png_read_ops               # noqa: E402
from univs_amd.evaluation import pvos, vps                # noqa: E402
from univs_amd.inference import png_read                  # noqa: E402

T = 20


def pillow_files(planes, palette=None):
    import io
    from PIL import Image
    out = []
    for p in planes:
        im = Image.fromarray(p)
        if palette is not None:
            im.putpalette(palette)
        buf = io.BytesIO()
        im.save(buf, format="PNG")
        out.append(buf.getvalue())
    return out


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


def readers(files, rgb, args, dev):
    """The three timings of one list of files."""
    from PIL import Image
    out = {"files": len(files), "file_bytes": sum(len(f) for f in files)}
    with tempfile.TemporaryDirectory() as root:
        paths = []
        for i, f in enumerate(files):
            paths.append(os.path.join(root, "%05d.png" % i))
            with open(paths[-1], "wb") as fh:
                fh.write(f)

        def host():
            planes = []
            for p in paths:
                with Image.open(p) as im:
                    planes.append(np.array(im.convert("RGB") if rgb and im.mode != "RGB" else im))
            return torch.as_tensor(np.stack(planes)).to(dev)

        def device():
            return torch.stack(png_read_ops.read_pngs_device(files, dev, rgb=rgb, uncovered="raise"))
        launches = []
        png_read_ops.read_covered([png_read.parse_png(f) for f in files], dev, rgb=rgb, launches=launches)
        s = alternate({"host": host, "device": device, "launches": launches[0]}, args.warmup, args.samples)
        out["planes_equal"] = bool(torch.equal(host(), device()))
    for k, key in (("host", "host_reader_ms"), ("device", "device_reader_ms"), ("launches", "launches_ms")):
        out[key] = bench.stats([v * 1e3 for v in s[k]], 3)
    out["device_faster_beyond_spread"] = out["device_reader_ms"]["max"] < out["host_reader_ms"]["min"]
    return out


def scorer(fn, args):
    s = alternate({"host": lambda: fn("host"), "gpu": lambda: fn("gpu")}, args.warmup, args.samples)
    out = {"host": bench.stats(s["host"], 4), "gpu": bench.stats(s["gpu"], 4)}
    out["gpu_faster_beyond_spread"] = out["gpu"]["max"] < out["host"]["min"]
    return out


def one(H, W, args, dev):
    out = {"frames": T, "size": [H, W]}
    ids, pred_ids = pvos_eval_bench.scene(T, H, W, 10)
    palette = [(37 * i + 11 * j) % 256 for i in range(256) for j in range(3)]
    vps_eval_bench.H, vps_eval_bench.W = H, W                        # (its scene is sized by its module constants)
    maps, gt_json, pred_json = vps_eval_bench.scene(0, 30)
    rgb = vps_eval_bench.rgb(maps["gt"])
    colours, seg = np.unique(maps["gt"], return_inverse=True)       # the panoptic ids are the packed colours
    lut, seg = vps_eval_bench.rgb(colours), seg.reshape(maps["gt"].shape).astype(np.uint8)
    written = {
        "palette_pillow": (pillow_files(ids, palette), False),
        "palette_gpu": (png_ops.png_files(png_ops.deflate_maps(torch.from_numpy(ids).to(dev)), H, W, 1, palette), False),
        "rgb_pillow": (pillow_files(rgb), True),
        "rgb_gpu": (png_ops.png_files(png_ops.deflate_maps(torch.from_numpy(seg).to(dev), torch.from_numpy(lut).to(dev), 3), H, W, 3), True),
    }
    for name, (files, is_rgb) in written.items():
        out[name] = readers(files, is_rgb, args, dev)
        print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    with tempfile.TemporaryDirectory() as root:
        data, res = pvos_eval_bench.write_tree(root, ids, pred_ids, 10)
        out["evaluate_pvos_files_s"] = scorer(lambda r: pvos.evaluate_pvos_files(res, data, eval_decay=True, device=dev, reader=r), args)
    with tempfile.TemporaryDirectory() as root:
        submit, truth, gt_file = vps_eval_bench.write_tree(root, maps, gt_json, pred_json)
        out["evaluate_vps_files_s"] = scorer(lambda r: vps.evaluate_vps_files(submit, truth, gt_file, device=dev, output_dir=os.path.join(root, "o"),
                                                                              reader=r), args)
    return out


def main():
    ap = bench.arg_parser(reps=1)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    dev = bench.gpu_or_exit("png_read_bench")
    out = {"device": torch.cuda.get_device_name(0), "samples": args.samples, "sizes": []}
    for H, W in ([(120, 214)] if args.quick else [(720, 1280), (1080, 1920)]):
        out["sizes"].append(one(H, W, args, dev))
    bench.emit(out, args.out)


if __name__ == "__main__":
    main()
