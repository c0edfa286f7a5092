"""Golden fixtures of the MinVIS-style video drivers (tests/golden/g24_*.npz): the reference's own
`InferenceVideoVISFast.inference_video_vis_minvis` (univs/inference/inference_video_vis_fast.py:219-351) and
`InferenceVideoVPS.inference_video_vps_online` (univs/inference/inference_video_vps.py:206-406) run on the CPU through
oracle.ref_harness, on the seeded closed-form head workloads.MinVISClipHead (query order shuffled per clip, objects entering and
leaving, one object reported by two queries in every other clip, stuff and thing classes with a repeated stuff class for VPS).

The model is replaced by its outputs: `backbone` returns the frames as its one feature map, `sem_seg_head` is the closed-form head.  The
reference's detectron2 stand-ins that the harness leaves inert are not reached (the drivers are entered below `eval`).

Each fixture stores the recipe (seed, sizes, settings), not the head's outputs -- the test regenerates them -- and the reference's
results, plus where they sit within rounding of a decision (the bounds the GPU tests allow differences in):
  VIS   scores, labels, the packed masks [N, V, H0, W0]; near0: pixels whose double-resized logit has |v| < 1e-5
  VPS   the panoptic map [V, H0, W0] (uint8), segments_infos, pred_ids; pan_tie: output pixels whose nearest source pixel has a
        top-two score x probability gap < 1e-6 or a |U_k| < 1e-5, or where some kept p_k = bilinear(sigmoid(U_k)) has |p_k - 0.5| < 1e-6

    python tools/gen_golden_minvis.py     # needs the reference tree (dev container only)
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from univs_amd.workloads import MinVISClipHead          # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOTAL_CLASSES = 3938                                     # rows of the CLIP class-embedding table

_VIS = dict(task="vis", h=16, w=24, padded=(64, 96), crop=(60, 90), out=(45, 68), Q=24, extra=4, num_queries=20, n_obj=6, window=5,
            topk=100, stability=0.0, zero_shot=False)
_VPS = dict(task="vps", dataset="vipseg", C=124, start=2924, h=16, w=24, padded=(64, 96), crop=(60, 88), out=(40, 60), Q=24, extra=4,
            num_queries=20, n_obj=7, window=2, topk=10, stability=0.0, object_mask=0.05, overlap=0.8,
            classes=[3, 7, 50, 50, 90, 12, 7], things=[4, 8, 13])
CASES = {
    "g24_vis_t2": dict(_VIS, seed=241, dataset="ovis", C=25, start=2243, V=9, T=2),
    "g24_vis_t3": dict(_VIS, seed=242, dataset="ytvis21", C=40, start=2203, V=9, T=3),
    "g24_vis_zero_shot": dict(_VIS, seed=243, dataset="ovis", C=25, start=2243, V=8, T=2, zero_shot=True, stability=0.02),
    "g24_vps_t2": dict(_VPS, seed=244, V=9, T=2),
    "g24_vps_t3": dict(_VPS, seed=245, V=9, T=3, overlap=0.5),
}


def make_head(r):
    return MinVISClipHead(r["seed"], r["V"], r["Q"], r["h"], r["w"], TOTAL_CLASSES, r["start"], r["C"], r["n_obj"], extra=r["extra"],
                          classes=r.get("classes"))


def stand_ins(r):
    """(model, batched_inputs, images, targets) of one recipe: what the drivers' clip loops read."""
    model = types.SimpleNamespace(backbone=lambda x: {"res2": x}, sem_seg_head=make_head(r))
    Hp, Wp = r["padded"]
    images = types.SimpleNamespace(tensor=torch.zeros(r["V"], 1, Hp, Wp), image_sizes=[tuple(r["crop"])] * r["V"])
    inputs = [{"dataset_name": r["dataset"], "height": r["out"][0], "width": r["out"][1], "video_id": 7, "video_len": r["V"]}]
    return model, inputs, images, [{}]


def reference_modules():
    from oracle import ref_harness
    ref_harness.ref_inference()
    import importlib
    return (importlib.import_module("univs.inference.inference_video_vis_fast"),
            importlib.import_module("univs.inference.inference_video_vps"))


def reference_driver(cls, r):
    obj = cls.__new__(cls)
    torch.nn.Module.__init__(obj)
    obj.__dict__.update(num_queries=r["num_queries"], stability_score_thresh=r["stability"], num_frames=r["T"],
                        num_frames_window_test=max(r["window"], r["T"]), merge_on_cpu=False, test_topk_per_image=r["topk"],
                        zero_shot_inference=r.get("zero_shot", False), object_mask_threshold=r.get("object_mask", 0.0),
                        overlap_threshold=r.get("overlap", 0.0), change_to_720p=True,
                        metadata=types.SimpleNamespace(thing_dataset_id_to_contiguous_id={c: c - 1 for c in r.get("things", [])}))
    obj.register_buffer("pixel_mean", torch.zeros(3, 1, 1), False)
    return obj


def pack(x):
    return np.packbits(np.asarray(x, dtype=bool).reshape(-1))


def resize(x, size):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)


def run_vis(m, r):
    obj = reference_driver(m.InferenceVideoVISFast, r)
    rec = {}
    save = obj.inference_video_vis_minvis_save_video

    def save_rec(model, images, outputs, interim_size, image_size, out_size):
        rec.update(outputs)
        return save(model, images, outputs, interim_size, image_size, out_size)
    obj.inference_video_vis_minvis_save_video = save_rec
    with torch.no_grad():
        res = obj.inference_video_vis_minvis(*stand_ins(r))
    masks = torch.stack([mk for mk in res["pred_masks"]]) if res["pred_masks"] else torch.zeros(0, r["V"], *r["out"], dtype=torch.bool)
    # near-zero double-resized logits: recovered per record as the row whose masks give its masks
    hi, wi = r["crop"]
    U = resize(rec["pred_masks"], r["padded"])[:, :, :hi, :wi]
    Vd = torch.stack([resize(u[None], r["out"])[0] for u in U])
    pos = Vd > 0
    near0 = torch.zeros(masks.shape, dtype=torch.bool)
    for i in range(masks.shape[0]):
        q = int(torch.nonzero((pos == masks[i]).flatten(1).all(1))[0])
        near0[i] = Vd[q].abs() < 1e-5
    return {"scores": np.asarray(res["pred_scores"], dtype=np.float32), "labels": np.asarray(res["pred_labels"], dtype=np.int64),
            "masks": pack(masks), "near0": pack(near0), "n": np.int64(masks.shape[0])}


def run_vps(m, r):
    obj = reference_driver(m.InferenceVideoVPS, r)
    rec = {}
    save = obj.inference_video_vps_save_results

    def save_rec(pred_cls, pred_masks, interim_size, img_size, out_size):
        rec.update(pred_cls=pred_cls, pred_masks=pred_masks, out_size=out_size)
        return save(pred_cls, pred_masks, interim_size, img_size, out_size)
    obj.inference_video_vps_save_results = save_rec
    with torch.no_grad():
        res = obj.inference_video_vps_online(*stand_ins(r))
    pan = res["pred_masks"]
    assert int(pan.max()) < 256
    # near-ties of the map, recomputed from the reference's inputs to its save step
    scores, labels = rec["pred_cls"].max(-1)
    keep = scores > max(r["object_mask"], scores.topk(k=r["topk"])[0][-1])
    hi, wi = r["crop"]
    U = resize(rec["pred_masks"][keep], r["padded"])[:, :, :hi, :wi]
    q = (U[:, ::5] > 1).flatten(1).sum(-1) / (U[:, ::5] > -1).flatten(1).sum(-1).clamp(min=1)
    sc = scores[keep] + 0.5 * q
    P = U.sigmoid()
    prob = sc.view(-1, 1, 1, 1) * P
    tie = (U.abs() < 1e-5).any(0)
    if prob.shape[0] > 1:
        t2 = prob.topk(2, dim=0)[0]
        tie |= (t2[0] - t2[1]) < 1e-6
    out = rec["out_size"]
    tie = F.interpolate(tie[None].float(), size=out, mode="nearest")[0] > 0
    for k in range(P.shape[0]):
        tie |= (resize(P[k][None], out)[0] - 0.5).abs() < 1e-6
    return {"pan": pan.numpy().astype(np.uint8), "pan_tie": pack(tie), "out_size": np.asarray(out, dtype=np.int64),
            "segments_infos": np.frombuffer(json.dumps(res["segments_infos"]).encode(), dtype=np.uint8),
            "pred_ids": np.asarray([int(v) for v in res["pred_ids"]], dtype=np.int64)}


def main():
    vis_m, vps_m = reference_modules()
    for name, r in CASES.items():
        d = run_vis(vis_m, r) if r["task"] == "vis" else run_vps(vps_m, r)
        d["recipe"] = np.frombuffer(json.dumps(r).encode(), dtype=np.uint8)
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **d)
        print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
