"""Times the first-frame masks of a VOS video on one MI355X and its host: the HIP kernel alone (run boundaries already on the
device), the wrapper including the upload of the boundaries, the whole GPU path of data.VOSTestMapper from the run-length codes
(`runs_from_rles`, one upload, one call), and what the reference does instead per object on one core -- `rle_decode`,
`PIL.Image.resize(NEAREST)`, the stack, the boxes from `any`, then the upload -- so that both ways end with the masks [N, Ho, Wo] and
the boxes [N, 4] on the device.  Reading the json is common to both and is not timed.

    python tools/prompt_masks_bench.py [--samples 5] [--warmup 2] [--reps 20] [--out profiles/prompt_masks_bench_v1.json]

`--samples` alternating samples per side, reported as median / min / max; a ratio is stated only where the two ranges do not overlap.
peak_extra_bytes is the allocator's peak during the wrapper's call above its inputs and outputs (the kernel has no workspace: 0 is
expected); host_stack_bytes is what the host path holds besides its result, the decoded full-resolution planes and the stack.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eval_bench_common as common  # noqa: E402
from univs_amd import prompts_ops, synth  # noqa: E402
from univs_amd.data.vos_mapper import bitmask_boxes  # noqa: E402
from univs_amd.evaluation.vis_counts import Runs, runs_from_rles  # noqa: E402
from univs_amd.inference.results import rle_decode, rle_encode_masks  # noqa: E402

CASES = [("480p_up_to_720p", 10, (480, 854), (720, 1280)), ("1080p_to_720p", 10, (1080, 1920), (720, 1280))]


def objects(name, N, H, W):
    """N masks of one frame as compressed run-length codes: each the union of three ellipses placed by the project's hash."""
    ys, xs = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    u = synth.hash_u01(f"prompt_masks_bench/{name}", N * 3 * 4).reshape(N, 3, 4)
    masks = np.zeros((N, H, W), bool)
    for i in range(N):
        for cy, cx, ry, rx in u[i]:
            masks[i] |= ((ys - cy * H) / (0.04 * H + ry * 0.2 * H)) ** 2 + ((xs - cx * W) / (0.04 * W + rx * 0.2 * W)) ** 2 <= 1.0
    return rle_encode_masks(torch.from_numpy(masks))


def bench_case(args, dev, name, N, in_hw, out_hw):
    from PIL import Image
    codes = objects(name, N, *in_hw)
    host_runs = runs_from_rles(codes, *in_hw)
    dev_runs = host_runs.to(dev)
    n = host_runs.starts.numel()

    def kernel():
        return prompts_ops.resize_rle_masks_u8(dev_runs, in_hw, out_hw)

    def upload_and_call(runs):
        packed = torch.cat([runs.starts, runs.bounds]).to(dev)
        return prompts_ops.resize_rle_masks_u8(Runs(packed[n:], None, packed[:n]), in_hw, out_hw)

    def wrapper_with_upload():
        return upload_and_call(host_runs)

    def gpu_path_from_codes():
        return upload_and_call(runs_from_rles(codes, *in_hw))

    def host_path_from_codes():
        planes = [np.asarray(Image.fromarray(rle_decode(c)).resize((out_hw[1], out_hw[0]), Image.NEAREST)) for c in codes]
        masks = torch.from_numpy(np.stack(planes))
        boxes = bitmask_boxes(masks.bool())
        return masks.to(dev), boxes.to(dev)

    sides = [("kernel", kernel, args.reps), ("wrapper_with_upload", wrapper_with_upload, 1), ("gpu_path_from_codes", gpu_path_from_codes, 1),
             ("host_path_from_codes", host_path_from_codes, 1)]
    for _ in range(args.warmup):
        for _, fn, _ in sides:
            fn()
    us = {k: [] for k, _, _ in sides}
    for _ in range(args.samples):
        for k, fn, reps in sides:
            us[k].append(common.sample(fn, reps))
    out = {"objects": N, "in_hw": list(in_hw), "out_hw": list(out_hw), "run_boundaries": int(host_runs.bounds.numel())}
    for k in us:
        out[f"{k}_us"] = common.stats(us[k])
    got, want = gpu_path_from_codes(), host_path_from_codes()
    out["equals_pillow"] = bool(torch.equal(got[0], want[0]) and torch.equal(got[1].float(), want[1]))
    del got, want
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = kernel()
    torch.cuda.synchronize()
    out["peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base - sum(t.numel() * t.element_size() for t in res))
    out["result_bytes"] = int(sum(t.numel() * t.element_size() for t in res))
    out["host_stack_bytes"] = int(N * in_hw[0] * in_hw[1] + N * out_hw[0] * out_hw[1])
    for side in ("wrapper_with_upload", "gpu_path_from_codes"):
        beyond = out[f"{side}_us"]["max"] < out["host_path_from_codes_us"]["min"]
        out[f"{side}_faster_than_host_path_beyond_spread"] = beyond
        if beyond:
            out[f"host_path_over_{side}"] = round(out["host_path_from_codes_us"]["median"] / out[f"{side}_us"]["median"], 2)
    return out


def main():
    args = common.arg_parser(reps=20).parse_args()
    dev = common.gpu_or_exit("prompt_masks_bench")
    import PIL
    out = {"tool": "prompt_masks_bench", "device": torch.cuda.get_device_name(0), "pillow": PIL.__version__, "samples": args.samples,
           "warmup": args.warmup, "kernel_reps": args.reps, "cases": {}}
    for name, N, in_hw, out_hw in CASES:
        out["cases"][name] = bench_case(args, dev, name, N, in_hw, out_hw)
    common.emit(out, args.out)


if __name__ == "__main__":
    main()
