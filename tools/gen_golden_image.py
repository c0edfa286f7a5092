"""Golden fixtures of the per-image post-processing (tests/golden/g23_*.npz): the reference's own
`InferenceImageGenericSegmentation.inference_image` (univs/inference/inference_image_generic_seg.py:207-431) run on the CPU through
oracle.ref_harness, on closed-form decoder outputs (workloads.image_blob_logits: Q' = 200 learnable + C text queries, so the reference's
`topk(k=200)` is legal).

The reference's third-party calls that the harness leaves inert are given their published semantics here:
  torchvision.ops.batched_nms   per-category by coordinate offset, greedy in descending score order (ties: ascending index), a box is
                                suppressed when IoU > threshold, area = (x2 - x1) * (y2 - y1)
  detectron2 sem_seg_postprocess  crop to the image size, bilinear (align_corners = False) to the output size
  detectron2 Instances / Boxes  plain attribute holders
The model is replaced by its outputs: `backbone` returns nothing, `sem_seg_head` returns the closed-form logits.

Each fixture stores the recipe (seed, sizes, settings), not the logits -- the test regenerates them -- and the reference's results:
the panoptic map and segments_info, the instances (packed masks, boxes, scores, classes), the sem_seg argmax and seeded samples of its
values, plus where the results sit within rounding of a decision (the bounds the GPU test allows differences in):
  pan_tie      pixels of the original size whose source pixel has a top-two score * sigmoid gap < 1e-6, or a winner with |U| < 1e-5
  inst_near0   instance pixels whose double-resized logit has |v| < 1e-5
  sem_tie      pixels whose top-two sem_seg values differ by < 1e-5 * max(1, |top|)

    python tools/gen_golden_image.py     # needs the reference tree (dev container only)
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

from univs_amd.workloads import image_blob_logits          # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOTAL_CLASSES = 3938                                       # rows of the CLIP class-embedding table

CASES = {
    # name: recipe.  coco_panoptic: the 80 thing classes are contiguous ids 0..79 (COCO panoptic's category order); ade20k: the
    # reference's metadata maps things AND stuff (ade20k_panoptic.py:186), so every class is a "thing" there.
    "g23_coco_panoptic": dict(seed=23, dataset="coco_panoptic", C=133, start=2641, Q=200, h=64, w=64, padded=256, crop=(192, 240),
                              out=(120, 150), things=list(range(80)), semantic_on=True, instance_on=True, panoptic_on=True,
                              overlap=0.8, object_mask=0.05, stability=0.0),
    "g23_ade20k": dict(seed=24, dataset="ade20k", C=150, start=2774, Q=200, h=64, w=64, padded=256, crop=(256, 171),
                       out=(144, 96), things=list(range(150)), semantic_on=True, instance_on=False, panoptic_on=True,
                       overlap=0.5, object_mask=0.02, stability=0.02),
}

NMS_RECORD = []


def batched_nms(boxes, scores, idxs, iou_threshold):
    """torchvision.ops.batched_nms, from its documentation (coordinate trick + greedy nms); kept in visiting order."""
    if boxes.numel() == 0:
        return torch.empty((0,), dtype=torch.int64)
    boxes = boxes + (idxs.to(boxes) * (boxes.max() + 1))[:, None]
    order = sorted(range(len(boxes)), key=lambda i: (-float(scores[i]), i))
    b = boxes.double()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    keep, removed = [], set()
    for a, i in enumerate(order):
        if i in removed:
            continue
        keep.append(i)
        for j in order[a + 1:]:
            if j in removed:
                continue
            iw = max(0.0, float(min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0])))
            ih = max(0.0, float(min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1])))
            inter = iw * ih
            union = float(area[i] + area[j]) - inter
            if union > 0 and inter / union > iou_threshold:
                removed.add(j)
    return torch.as_tensor(keep, dtype=torch.int64)


def sem_seg_postprocess(result, img_size, output_height, output_width):
    result = result[:, : img_size[0], : img_size[1]].expand(1, -1, -1, -1)
    return F.interpolate(result, size=(output_height, output_width), mode="bilinear", align_corners=False)[0]


class _Holder:
    def __init__(self, *a, **k):
        if a and not k and len(a) == 1 and isinstance(a[0], torch.Tensor):
            self.tensor = a[0].float()
        else:
            self.image_size = a[0] if a else None


def reference_module():
    from oracle import ref_harness
    ref_harness.ref_inference()
    sys.modules["univs.inference.visualization"].display_instance_masks = None
    import importlib
    m = importlib.import_module("univs.inference.inference_image_generic_seg")
    m.batched_nms = batched_nms
    m.sem_seg_postprocess = sem_seg_postprocess
    m.Instances = _Holder
    m.Boxes = _Holder
    return m


def decoder_outputs(r):
    Qp = r["Q"] + r["C"]
    lowres_crop = (r["crop"][0] * r["h"] // r["padded"], r["crop"][1] * r["w"] // r["padded"])
    L, cls = image_blob_logits(r["seed"], Qp, r["h"], r["w"], r["C"], lowres_crop)
    return L, cls


def run_case(m, r):
    L, cls = decoder_outputs(r)
    Qp = L.shape[0]
    full = torch.full((1, Qp, TOTAL_CLASSES), -20.0)
    full[0, :, r["start"]:r["start"] + r["C"]] = cls
    outputs = {"pred_logits": full, "pred_masks": L[None, :, None], "pred_reid_logits": torch.zeros(1, Qp, 4), "aux_outputs": []}
    model = types.SimpleNamespace(backbone=lambda x: None, sem_seg_head=lambda feats, targets=None: dict(outputs))
    meta = types.SimpleNamespace(thing_dataset_id_to_contiguous_id={i + 1: c for i, c in enumerate(r["things"])})
    obj = m.InferenceImageGenericSegmentation.__new__(m.InferenceImageGenericSegmentation)
    torch.nn.Module.__init__(obj)
    obj.__dict__.update(num_queries=r["Q"], object_mask_threshold=r["object_mask"], overlap_threshold=r["overlap"],
                        stability_score_thresh=r["stability"], metadata=meta, sem_seg_postprocess_before_inference=False,
                        prompt_as_queries=True, disable_semantic_queries=False, semantic_on=r["semantic_on"], instance_on=r["instance_on"],
                        panoptic_on=r["panoptic_on"], test_topk_per_image=100)
    obj.register_buffer("pixel_mean", torch.zeros(3, 1, 1), False)
    # the inputs of panoptic_inference's argmax, recorded from its NMS (biou 0.9) to find the near-ties of the map
    nms_orig = obj.postprocess_nms

    def nms_rec(scores, mask_pred, box_pred=None, biou_threshold=0.85):
        out = nms_orig(scores, mask_pred, box_pred, biou_threshold)
        NMS_RECORD.append((biou_threshold, out[0], out[1]))
        return out
    obj.postprocess_nms = nms_rec
    P = r["padded"]
    images = types.SimpleNamespace(tensor=torch.zeros(1, 3, P, P), image_sizes=[tuple(r["crop"])])
    inputs = [{"dataset_name": r["dataset"], "height": r["out"][0], "width": r["out"][1]}]
    NMS_RECORD.clear()
    with torch.no_grad():
        res = obj.inference_image(model, inputs, images, None)[0]
    return L, res


def pack(x):
    return np.packbits(np.asarray(x, dtype=bool).reshape(-1))


def main():
    m = reference_module()
    for name, r in CASES.items():
        L, res = run_case(m, r)
        H0, W0 = r["out"]
        d = {"recipe": np.frombuffer(json.dumps(r).encode(), dtype=np.uint8)}
        U = F.interpolate(L[None], size=(r["padded"], r["padded"]), mode="bilinear", align_corners=False)[0]
        hi, wi = r["crop"]
        if r["panoptic_on"]:
            pan, info = res["panoptic_seg"]
            d["pan"] = pan.numpy().astype(np.int32)
            d["pan_info"] = np.frombuffer(json.dumps(info).encode(), dtype=np.uint8)
            thr, mc, mp = [x for x in NMS_RECORD if x[0] == 0.9][0]
            s, _ = mc.max(-1)
            keep = s > r["object_mask"]
            sc = (mc / 0.06).softmax(-1).max(-1)[0][keep]
            logit = mp[keep]
            prob = sc.view(-1, 1, 1) * logit.sigmoid()
            top2 = prob.topk(2, dim=0) if prob.shape[0] > 1 else None
            tie = (top2[0][0] - top2[0][1] < 1e-6) if top2 is not None else torch.zeros(hi, wi, dtype=torch.bool)
            win = logit.gather(0, prob.argmax(0)[None])[0]
            tie = tie | (win.abs() < 1e-5)
            tie = F.interpolate(tie[None, None].float(), size=(H0, W0), mode="nearest")[0, 0] > 0
            d["pan_tie"] = pack(tie)
        if r["instance_on"]:
            inst = res["instances"]
            masks = inst.pred_masks > 0
            d["inst_masks"] = pack(masks)
            d["inst_boxes"] = inst.pred_boxes.tensor.numpy().astype(np.float32)
            d["inst_scores"] = inst.scores.numpy().astype(np.float32)
            d["inst_classes"] = inst.pred_classes.numpy().astype(np.int64)
            # near-zero logits of the kept instances: recovered per instance as the plane whose double resize gives its mask
            near0 = torch.zeros(masks.shape, dtype=torch.bool)
            Uc = U[:, :hi, :wi]
            V = F.interpolate(Uc[None], size=(H0, W0), mode="bilinear", align_corners=False)[0] if (hi, wi) != (H0, W0) else Uc
            pos = V > 0
            for i in range(masks.shape[0]):
                q = int(torch.nonzero((pos == masks[i]).flatten(1).all(1))[0])
                near0[i] = V[q].abs() < 1e-5
            d["inst_near0"] = pack(near0)
        if r["semantic_on"]:
            sem = res["sem_seg"]
            d["sem_argmax"] = sem.argmax(0).numpy().astype(np.int16)
            t2 = sem.topk(2, dim=0)[0]
            d["sem_tie"] = pack((t2[0] - t2[1]) < 1e-5 * t2[0].abs().clamp(min=1))
            rs = np.random.RandomState(r["seed"])
            idx = np.stack([rs.randint(0, sem.shape[0], 4096), rs.randint(0, H0, 4096), rs.randint(0, W0, 4096)], 1)
            d["sem_idx"] = idx.astype(np.int32)
            d["sem_val"] = sem[idx[:, 0], idx[:, 1], idx[:, 2]].numpy().astype(np.float32)
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **d)
        print(path, os.path.getsize(path), "bytes;", {k: v.shape for k, v in d.items()})


if __name__ == "__main__":
    main()
