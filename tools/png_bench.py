"""Times the result PNGs of a video on one MI355X and its host, both ways: png="gpu" (csrc/png_deflate.hip emits every frame's zlib
stream, the host wraps it in chunks) against the parent's path (the planes are downloaded, `Image.fromarray`, `putpalette`, `save`:
zlib level 6 on one host core).  Three levels: the kernels alone (maps on the device, buffers allocated, nothing downloaded), the
wrapper with its two downloads against download + Pillow into memory, and the writers of inference/results.py end to end with the file
writes (`write_vos_pngs` for the palette map, `write_vps_predictions` for the panoptic map, whose host side also paints the RGB planes
and both sides compute the segment records).

    python tools/png_bench.py [--samples 5] [--warmup 2] [--reps 20] [--out profiles/png_encode_bench_v1.json]

`--samples` alternating samples per side, reported as median / min / max; a ratio is stated only where the two ranges do not overlap,
and a case where the device path is slower says so.  File sizes of both ways are reported, not bounded: the fixed Huffman code with
run matches only gives larger files than zlib level 6.  peak_extra_bytes is the allocator's peak during the wrapper's device call
above its inputs and outputs: the scratch slots, sized for the worst case.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_bench_common as common  # noqa: E402
from univs_amd import png_ops, synth  # noqa: E402
from univs_amd.inference import results  # noqa: E402

FRAMES = 20
CASES = [("palette_720p", "palette", 10, (720, 1280)), ("palette_1080p", "palette", 10, (1080, 1920)),
         ("panoptic_720p", "panoptic", 30, (720, 1280)), ("panoptic_1080p", "panoptic", 30, (1080, 1920))]
PALETTE = [(i * 37 + j * 11) % 256 for i in range(256) for j in range(3)]
CATEGORIES = {c: {"id": c, "isthing": int(c % 3 == 0), "color": [(c * 40 + 9) % 256, (c * 70 + 20) % 256, (c * 110 + 5) % 256]}
              for c in range(1, 41)}


def id_maps(name, n_ids, H, W):
    """uint8 [FRAMES, H, W]: n_ids ellipses placed by the project's hash, drifting a little from frame to frame; 0 is background."""
    u = synth.hash_u01(f"png_bench/{name}", n_ids * 6).reshape(n_ids, 6)
    out = np.zeros((FRAMES, H, W), np.uint8)
    for t in range(FRAMES):
        for i, (cy, cx, ry, rx, vy, vx) in enumerate(u):
            y0, x0 = (cy + 0.004 * t * (vy - 0.5)) * H, (cx + 0.004 * t * (vx - 0.5)) * W
            ay, ax = 0.04 * H + ry * 0.2 * H, 0.04 * W + rx * 0.2 * W
            ya, yb, xa, xb = max(int(y0 - ay), 0), min(int(y0 + ay) + 2, H), max(int(x0 - ax), 0), min(int(x0 + ax) + 2, W)
            if ya >= yb or xa >= xb:
                continue
            ys, xs = np.arange(ya, yb, dtype=np.float64)[:, None], np.arange(xa, xb, dtype=np.float64)[None, :]
            out[t, ya:yb, xa:xb][((ys - y0) / ay) ** 2 + ((xs - x0) / ax) ** 2 <= 1.0] = i + 1
    return out


def _pillow_bytes(plane, palette=None):
    import io
    from PIL import Image
    img = Image.fromarray(plane)
    if palette is not None:
        img.putpalette(palette)
    buf = io.BytesIO()
    img.save(buf, format="PNG")
    return buf.getvalue()


def bench_case(args, dev, name, kind, n_ids, hw):
    H, W = hw
    maps = id_maps(name, n_ids, H, W)
    names = [f"video/{t:05d}.jpg" for t in range(FRAMES)]
    root = tempfile.mkdtemp(prefix="png_bench_")
    if kind == "palette":
        ids, lut_host, lut, C, palette = torch.from_numpy(maps).to(dev), None, None, 1, PALETTE
    else:
        infos = [{"id": i + 1, "isthing": bool(CATEGORIES[i + 1]["isthing"]), "category_id": i + 1} for i in range(n_ids)]
        lut_host = np.zeros((n_ids + 1, 3), np.uint8)
        for info in infos:
            lut_host[info["id"]] = CATEGORIES[info["category_id"]]["color"]
        ids, lut, C, palette = torch.from_numpy(maps.astype(np.int32)).to(dev), torch.from_numpy(lut_host).to(dev), 3, None
        inputs = {"file_names": names, "frame_indices": list(range(FRAMES)), "video_id": "video"}
        outputs = {"image_size": (H, W), "pred_masks": ids, "segments_infos": infos}

    def kernels():
        return png_ops.deflate_maps_device(ids, lut, C)

    def wrapper():
        return png_ops.png_files(png_ops.deflate_maps(ids, lut, C), H, W, C, palette)

    def pillow():
        planes = ids.cpu().numpy()
        planes = planes.astype(np.uint8) if lut_host is None else lut_host[planes]
        return [_pillow_bytes(p, palette) for p in planes]

    if kind == "palette":
        def writer_gpu():
            return results.write_vos_pngs(os.path.join(root, "g"), names, 0, ids, palette, png="gpu")

        def writer_host():
            return results.write_vos_pngs(os.path.join(root, "h"), names, 0, ids, palette)
    else:
        def writer_gpu():
            return results.write_vps_predictions(inputs, outputs, os.path.join(root, "g"), CATEGORIES, png="gpu")

        def writer_host():
            return results.write_vps_predictions(inputs, outputs, os.path.join(root, "h"), CATEGORIES)

    sides = [("kernels", kernels, args.reps), ("wrapper_with_downloads", wrapper, 1), ("download_and_pillow", pillow, 1),
             ("writer_gpu", writer_gpu, 1), ("writer_host", writer_host, 1)]
    try:
        for _ in range(args.warmup):
            for _, fn, _ in sides:
                fn()
        us = {k: [] for k, _, _ in sides}
        for _ in range(args.samples):
            for k, fn, reps in sides:
                us[k].append(common.sample(fn, reps))
        out = {"frames": FRAMES, "hw": list(hw), "ids": n_ids, "channels": C}
        for k in us:
            out[f"{k}_us"] = common.stats(us[k])
        ours, theirs = wrapper(), pillow()
        from PIL import Image
        import io
        out["decodes_equal"] = bool(all(np.array_equal(np.asarray(Image.open(io.BytesIO(a))), np.asarray(Image.open(io.BytesIO(b))))
                                        for a, b in zip(ours, theirs)))
        out["file_bytes_gpu"] = common.stats([len(a) for a in ours], 0)
        out["file_bytes_pillow"] = common.stats([len(b) for b in theirs], 0)
        del ours, theirs
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = kernels()
        torch.cuda.synchronize()
        held = sum(t.numel() * t.element_size() for t in res)
        out["peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base - held)
        out["output_buffer_bytes"] = int(held)
        out["stream_bytes"] = int(res[1][-1])
        for ours_k, theirs_k in (("wrapper_with_downloads", "download_and_pillow"), ("writer_gpu", "writer_host")):
            beyond = out[f"{ours_k}_us"]["max"] < out[f"{theirs_k}_us"]["min"]
            out[f"{ours_k}_faster_beyond_spread"] = beyond
            out[f"{ours_k}_slower"] = out[f"{ours_k}_us"]["median"] > out[f"{theirs_k}_us"]["median"]
            if beyond:
                out[f"{theirs_k}_over_{ours_k}"] = round(out[f"{theirs_k}_us"]["median"] / out[f"{ours_k}_us"]["median"], 2)
        return out
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = common.arg_parser(reps=20)
    ap.add_argument("--cases", default=None, help="comma-separated case names (default: all)")
    args = ap.parse_args()
    dev = common.gpu_or_exit("png_bench")
    import PIL
    out = {"tool": "png_bench", "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__, "samples": args.samples,
           "warmup": args.warmup, "kernel_reps": args.reps, "cases": {}}
    for name, kind, n_ids, hw in CASES:
        if args.cases is None or name in args.cases.split(","):
            out["cases"][name] = bench_case(args, dev, name, kind, n_ids, hw)
    common.emit(out, args.out)


if __name__ == "__main__":
    main()
