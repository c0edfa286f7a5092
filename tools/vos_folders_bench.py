"""Times the prompts of a VOS video made from its annotation PNGs on one MI355X and its host: the census launch and the prompts call
alone (id maps already on the device), the wrapper including the upload of the id maps, and the mask step of data.VOSTestMapper from
the PNG files with resize="gpu" (Pillow decodes the PNGs; and with decode="gpu", where png_read_ops does) -- alternated with (a) the
same step with resize="host" (Pillow per object, the boxes from `any`, then the upload) and (b) the json route's `_gpu_masks` on the same masks as run-length codes (`runs_from_rles`, one upload,
csrc/mask_prompt_resize.hip), which is the fastest way to the same tensors without this route.  All three end with the masks
[N, Ho, Wo] and the boxes [N, 4] on the device.  Making the records (listing folders, reading meta files) is not timed.

    python tools/vos_folders_bench.py [--samples 5] [--warmup 2] [--reps 20] [--out profiles/vos_folders_bench_v1.json]

`--samples` alternating samples per side, reported as median / min / max; a ratio is stated only where the two ranges do not overlap.
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_bench_common as common  # noqa: E402
from univs_amd import idmap_ops, synth  # noqa: E402
from univs_amd.data import VOSTestMapper  # noqa: E402
from univs_amd.inference.results import rle_encode_masks  # noqa: E402

N_OBJECTS = 10
CASES = [("480p_up_to_720p_1_frame", 1, (480, 854), (720, 1280)), ("480p_up_to_720p_5_frames", 5, (480, 854), (720, 1280)),
         ("1080p_to_720p_1_frame", 1, (1080, 1920), (720, 1280)), ("1080p_to_720p_5_frames", 5, (1080, 1920), (720, 1280))]
NAME = "sot_sot_davis17_val"


def idmap(name, N, H, W):
    """uint8 [H, W]: N objects, values 1 .. N, each the union of three ellipses placed by the project's hash, later ones on top."""
    ys, xs = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    u = synth.hash_u01(f"vos_folders_bench/{name}", N * 3 * 4).reshape(N, 3, 4)
    m = np.zeros((H, W), np.uint8)
    for i in range(N):
        for cy, cx, ry, rx in u[i]:
            m[((ys - cy * H) / (0.04 * H + ry * 0.2 * H)) ** 2 + ((xs - cx * W) / (0.04 * W + rx * 0.2 * W)) ** 2 <= 1.0] = i + 1
    return m


def bench_case(args, dev, folder, name, F, in_hw, out_hw):
    from PIL import Image
    maps = np.stack([idmap(f"{name}/{f}", N_OBJECTS, *in_hw) for f in range(F)])
    folder_frames, json_frames, frame, value = [], [], [], []
    for f in range(F):
        path = os.path.join(folder, f"{name}_{f:05d}.png")
        im = Image.fromarray(maps[f], mode="P")
        im.putpalette([0, 0, 0, 128, 0, 0, 0, 128, 0] + [0] * 759)
        im.save(path)
        present = [v for v in range(1, N_OBJECTS + 1) if (maps[f] == v).any()]
        codes = rle_encode_masks(torch.from_numpy(np.stack([maps[f] == v for v in present])))
        folder_frames.append([{"png": path, "value": v} for v in present])
        json_frames.append([{"segmentation": c} for c in codes])
        frame += [f] * len(present)
        value += present
    ids_d, frame_d, value_d = idmap_ops.upload_prompts(maps, frame, value, dev)
    gpu_mapper, host_mapper = VOSTestMapper(720, 1280, resize="gpu", device=dev), VOSTestMapper(720, 1280, resize="host")
    decode_mapper = VOSTestMapper(720, 1280, resize="gpu", device=dev, decode="gpu")

    def census_kernel():
        return idmap_ops.idmap_census_u8(ids_d)

    def prompts_kernel():
        return idmap_ops.idmap_prompts_u8(ids_d, frame_d, value_d, out_hw)

    def wrapper_with_upload():
        return idmap_ops.idmap_prompts_u8(*idmap_ops.upload_prompts(maps, frame, value, dev), out_hw)

    def mapper_gpu_from_pngs():
        gpu_mapper._idmaps = {}
        return gpu_mapper._gpu_idmap_masks(folder_frames, in_hw, out_hw, name, NAME)

    def mapper_gpu_decode_gpu_from_pngs():
        return decode_mapper._gpu_idmap_masks(folder_frames, in_hw, out_hw, name, NAME)

    def mapper_host_from_pngs():
        host_mapper._idmaps = {}
        return [(m.to(dev), b.to(dev)) for m, b in (host_mapper._host_masks(objs, out_hw, NAME) for objs in folder_frames)]

    def json_route_gpu_masks():
        return gpu_mapper._gpu_masks(json_frames, in_hw, out_hw, name)

    sides = [("census_kernel", census_kernel, args.reps), ("prompts_kernel", prompts_kernel, args.reps), ("wrapper_with_upload", wrapper_with_upload, 1),
             ("mapper_gpu_from_pngs", mapper_gpu_from_pngs, 1), ("mapper_gpu_decode_gpu_from_pngs", mapper_gpu_decode_gpu_from_pngs, 1),
             ("mapper_host_from_pngs", mapper_host_from_pngs, 1),
             ("json_route_gpu_masks", json_route_gpu_masks, 1)]
    for _ in range(args.warmup):
        for _, fn, _ in sides:
            fn()
    us = {k: [] for k, _, _ in sides}
    for _ in range(args.samples):
        for k, fn, reps in sides:
            us[k].append(common.sample(fn, reps))
    out = {"objects": len(frame), "annotated_frames": F, "in_hw": list(in_hw), "out_hw": list(out_hw)}
    for k in us:
        out[f"{k}_us"] = common.stats(us[k])
    got, want, other = mapper_gpu_from_pngs(), mapper_host_from_pngs(), json_route_gpu_masks()
    out["equals_pillow"] = bool(all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, want)))
    out["decode_gpu_equals"] = bool(all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, mapper_gpu_decode_gpu_from_pngs())))
    out["equals_json_route"] = bool(all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(got, other)))
    out["source_bytes"] = int(maps.size)
    out["result_bytes"] = int(len(frame) * out_hw[0] * out_hw[1])
    out["prompts_kernel_GBps"] = round((out["source_bytes"] + out["result_bytes"]) / (out["prompts_kernel_us"]["median"] * 1e-6) / 1e9, 1)
    out["census_kernel_GBps"] = round(out["source_bytes"] / (out["census_kernel_us"]["median"] * 1e-6) / 1e9, 1)
    for other_side in ("mapper_host_from_pngs", "json_route_gpu_masks"):
        a, b = out["mapper_gpu_from_pngs_us"], out[f"{other_side}_us"]
        beyond = a["max"] < b["min"] or b["max"] < a["min"]
        out[f"differs_from_{other_side}_beyond_spread"] = beyond
        if beyond:
            out[f"{other_side}_over_mapper_gpu_from_pngs"] = round(b["median"] / a["median"], 2)
    return out


def main():
    args = common.arg_parser(reps=20).parse_args()
    dev = common.gpu_or_exit("vos_folders_bench")
    import PIL
    out = {"tool": "vos_folders_bench", "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__, "samples": args.samples,
           "warmup": args.warmup, "kernel_reps": args.reps, "cases": {}}
    with tempfile.TemporaryDirectory() as folder:
        for name, F, in_hw, out_hw in CASES:
            out["cases"][name] = bench_case(args, dev, folder, name, F, in_hw, out_hw)
    common.emit(out, args.out)


if __name__ == "__main__":
    main()
