"""Golden fixtures of the semantic-extraction driver (tests/golden/g25_semantic_*.npz): the reference's own
`InferenceVideoSemanticExtraction.inference_video` (univs/inference/inference_video_semantic_extraction.py:181-262) run on the CPU
through oracle.ref_harness, on the seeded closed-form head workloads.SemanticClipHead, into a temporary directory; the two `.pt` files
are read back.

The model is replaced by its outputs: `backbone` returns the frames as its one feature map, `sem_seg_head` is the closed-form head.  The
driver is entered below `eval` (no `prepare_targets`).

Each fixture stores the recipe (seed, sizes, settings), not the head's outputs -- the test regenerates them -- and what the reference
made of them: the two file names, the list of head calls (first_frame_idx, frame_indices, frames handed in) and the two saved tensors.

The cases cover: a video that is not a multiple of the clip length (a shorter last clip), videos spanning more than one backbone window,
temporal ratios whose kept frames are not the first frame of their clip, a crop smaller than the padded size in both axes, output sizes
larger and smaller than the crop and the default one, truncating int(out / ratio), ratio 32 on a 720 x 1280 output, and widths that are
not a multiple of 4.

    python tools/gen_golden_semantic.py     # needs the reference tree (dev container only)
"""
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from univs_amd.workloads import SemanticClipHead         # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")

CASES = {
    # out smaller than the crop; 45 / 8 and 68 / 8 truncate; V = 8 = 2 clips + a 2-frame clip, two backbone windows (6 + 2 frames)
    "g25_semantic_r8": dict(seed=251, C=8, N=5, h=16, w=24, padded=(64, 96), crop=(60, 90), out=(45, 68), ratio=8, t_itv=1, T=3, V=8,
                            video_id="vid_r8", default_dir=False),
    # ratio 32 on a 720 x 1280 output (22 x 40; 720 / 32 truncates), out larger than the crop; t_itv = 3 keeps frames 0 and 3, frame 3 the
    # second frame of clip [2, 3]; V = 5 = 2 clips + a 1-frame clip, two windows (4 + 1 frames); the default output directory
    "g25_semantic_r32_720p": dict(seed=252, C=8, N=5, h=24, w=40, padded=(96, 160), crop=(90, 158), out=(720, 1280), ratio=32, t_itv=3, T=2,
                                  V=5, video_id="vid_r32", default_dir=True),
    # out larger than the crop; 151 / 8 truncates to 18 (not a multiple of 4); t_itv = 2 keeps frame 4, the second of clip [3, 4, 5];
    # V = 10 = 3 clips + a 1-frame clip, two windows (6 + 4 frames)
    "g25_semantic_t3": dict(seed=253, C=8, N=5, h=20, w=28, padded=(80, 112), crop=(75, 101), out=(120, 151), ratio=8, t_itv=2, T=3, V=10,
                            video_id="vid_t3", default_dir=False),
    # no height / width in the record: the un-padded image size (60 x 90 -> 7 x 11); V a multiple of T, one window
    "g25_semantic_default_size": dict(seed=254, C=8, N=5, h=16, w=24, padded=(64, 96), crop=(60, 90), out=None, ratio=8, t_itv=1, T=2, V=4,
                                      video_id="vid_default", default_dir=False),
}


def stand_ins(r, root):
    """(model, batched_inputs, images, targets) of one recipe: what the driver's clip loop reads.  `root`: where the frames pretend to be."""
    head = SemanticClipHead(r["seed"], r["C"], r["N"], r["h"], r["w"])
    model = types.SimpleNamespace(backbone=lambda x: {"res2": x}, sem_seg_head=head)
    Hp, Wp = r["padded"]
    images = types.SimpleNamespace(tensor=torch.zeros(r["V"], 1, Hp, Wp), image_sizes=[tuple(r["crop"])] * r["V"])
    inputs = [{"video_id": r["video_id"], "video_len": r["V"]}]
    if r["out"] is not None:
        inputs[0].update(height=r["out"][0], width=r["out"][1])
    targets = [{"file_names": [f"{root}/raw/set1/{r['video_id']}/{i:05d}.jpg" for i in range(r["V"])]}]
    return model, inputs, images, targets


def expected_dir(r, root, out_dir):
    return out_dir if not r["default_dir"] else f"{root}/raw/set1".replace("raw", "semantic_extraction")


def reference_driver(cls, r, out_dir):
    obj = cls.__new__(cls)
    torch.nn.Module.__init__(obj)
    obj.__dict__.update(num_frames=r["T"], num_frames_window_test=2 * r["T"], semantic_extraction_enable=True,
                        semantic_extraction_compression_ratio=r["ratio"], semantic_extraction_compression_ratio_temporal=r["t_itv"],
                        semantic_extraction_output_dir="" if r["default_dir"] else out_dir)
    obj.register_buffer("pixel_mean", torch.zeros(3, 1, 1), False)
    return obj


def run(m, r):
    with tempfile.TemporaryDirectory() as root:
        out_dir = os.path.join(root, "out")
        obj = reference_driver(m.InferenceVideoSemanticExtraction, r, out_dir)
        model, inputs, images, targets = stand_ins(r, root)
        with torch.no_grad():
            assert obj.inference_video(model, inputs, images, targets) is None
        where = expected_dir(r, root, out_dir)
        names = sorted(os.listdir(where))
        assert len(names) == 2, names
        feats, toks = (torch.load(os.path.join(where, n)) for n in names)      # '._compression...' sorts before '._obj_tokens...'
    return {"names": np.frombuffer(json.dumps(names).encode(), dtype=np.uint8),
            "calls": np.frombuffer(json.dumps(model.sem_seg_head.calls).encode(), dtype=np.uint8),
            "obj_tokens": toks.contiguous().numpy(), "features": feats.contiguous().numpy()}


def main():
    from oracle import ref_harness
    ref_harness.ref_inference()
    m = importlib.import_module("univs.inference.inference_video_semantic_extraction")
    for name, r in CASES.items():
        d = run(m, r)
        d["recipe"] = np.frombuffer(json.dumps(r).encode(), dtype=np.uint8)
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **d)
        print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
