"""Times the test-time resize of a video's frames on one MI355X and its host: the HIP kernel alone (frames already on the device), the
wrapper including the upload of the decoded frames, and what the host path does instead -- `PIL.Image.resize` per frame on one core
(Pillow's resize runs on the calling thread), alone and followed by the transpose and the upload of the resized frames, so that both
ways end with uint8 [T, 3, Ho, Wo] on the device.  Decoding the files is common to both and is not timed.

    python tools/frames_bench.py [--samples 5] [--warmup 2] [--reps 20] [--out profiles/frame_resize_bench_v1.json]

`--samples` alternating samples per side, reported as median / min / max; a ratio is stated only where the two ranges do not overlap.
kernel_GBps is the bytes the algorithm has to move, T (Hi Wi + Ho Wo) 3, over the kernel's median time, beside the 8 TB/s the HBM can
give; what the kernel re-reads from cache is not in it.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_bench_common as common  # noqa: E402
from univs_amd import frames_ops, synth  # noqa: E402
from univs_amd.data.mapper import _pil_resize  # noqa: E402

CASES = [("1080p_to_720p", 20, (1080, 1920), (720, 1280)), ("480p_up_to_720p", 20, (480, 854), (720, 1280))]
HBM_GBPS = 8000.0


def bench_case(args, dev, name, T, in_hw, out_hw):
    host = np.floor(synth.hash_u01(f"frames_bench/{name}", T * in_hw[0] * in_hw[1] * 3) * 256.0).astype(np.uint8).reshape(T, *in_hw, 3)
    on_dev = torch.from_numpy(host).to(dev)

    def kernel():
        return frames_ops.resize_frames_u8(on_dev, out_hw)

    def wrapper_with_upload():
        return frames_ops.resize_frames_u8(torch.from_numpy(host).to(dev), out_hw)

    def pillow():
        return [_pil_resize(f, *out_hw) for f in host]

    def pillow_then_upload():
        return torch.from_numpy(np.stack([_pil_resize(f, *out_hw).transpose(2, 0, 1) for f in host])).to(dev)

    sides = [("kernel", kernel, args.reps), ("wrapper_with_upload", wrapper_with_upload, 1), ("pillow_one_core", pillow, 1),
             ("pillow_then_upload", pillow_then_upload, 1)]
    for _ in range(args.warmup):
        for _, fn, _ in sides:
            fn()
    us = {k: [] for k, _, _ in sides}
    for _ in range(args.samples):
        for k, fn, reps in sides:
            us[k].append(common.sample(fn, reps))
    out = {"frames": T, "in_hw": list(in_hw), "out_hw": list(out_hw)}
    for k in us:
        out[f"{k}_us"] = common.stats(us[k])
    moved = T * 3 * (in_hw[0] * in_hw[1] + out_hw[0] * out_hw[1])
    out["algorithmic_bytes"] = moved
    out["kernel_GBps"] = round(moved / (out["kernel_us"]["median"] * 1e-6) / 1e9, 1)
    out["kernel_share_of_hbm_peak"] = round(out["kernel_GBps"] / HBM_GBPS, 4)
    out["upload_share_of_wrapper"] = round(1.0 - out["kernel_us"]["median"] / out["wrapper_with_upload_us"]["median"], 3)
    out["equals_pillow"] = bool(torch.equal(wrapper_with_upload(), pillow_then_upload()))
    out["wrapper_faster_than_pillow_then_upload_beyond_spread"] = out["wrapper_with_upload_us"]["max"] < out["pillow_then_upload_us"]["min"]
    if out["wrapper_faster_than_pillow_then_upload_beyond_spread"]:
        out["pillow_then_upload_over_wrapper"] = round(out["pillow_then_upload_us"]["median"] / out["wrapper_with_upload_us"]["median"], 2)
    return out


def main():
    args = common.arg_parser(reps=20).parse_args()
    dev = common.gpu_or_exit("frames_bench")
    import PIL
    out = {"tool": "frames_bench", "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__, "samples": args.samples,
           "warmup": args.warmup, "kernel_reps": args.reps, "hbm_peak_GBps": HBM_GBPS, "cases": {}}
    for name, T, in_hw, out_hw in CASES:
        out["cases"][name] = bench_case(args, dev, name, T, in_hw, out_hw)
    common.emit(out, args.out)


if __name__ == "__main__":
    main()
