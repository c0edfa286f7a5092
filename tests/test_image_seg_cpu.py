"""CPU: the per-image driver (univs_amd/inference/image_generic_seg.py) -- config keys, the dispatch of `UniVS_Prompt.forward_inference`,
the NMS restatement, the panoptic segment table, the nearest-index rule, and a COCO-panoptic image end to end through the model on the
oracle's CPU operators."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.cpu_path import cpu_ops
from tests import cases
from univs_amd import synth
from univs_amd.config import get_cfg
from univs_amd.inference.image_generic_seg import (AtenSteps, InferenceImageGenericSegmentation, batched_nms, nearest_source_index, nms,
                                                   panoptic_segments)
from univs_amd.modeling.build import build_model
from univs_amd.workloads import image_blob_logits


def image_cfg(**test_over):
    cfg = get_cfg()
    cfg.INPUT.SAMPLING_FRAME_NUM = 1
    cfg.INPUT.LSJ_AUG.IMAGE_SIZE = 128
    cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES = 20
    cfg.MODEL.UniVS.CLIP_CLASS_EMBED_PATH = cases.clip_table()
    cfg.MODEL.MASK_FORMER.TEST.OVERLAP_THRESHOLD = 0.8
    cfg.MODEL.MASK_FORMER.TEST.OBJECT_MASK_THRESHOLD = 0.05
    for k, v in test_over.items():
        cfg.MODEL.MASK_FORMER.TEST[k] = v
    return cfg


def image_input(dataset, H=96, W=120, height=60, width=75):
    return [{"image": synth.synthetic_frames(1, H, W, "image/frames"), "height": height, "width": width, "task": "detection",
             "dataset_name": dataset, "file_names": ["img/0.jpg"], "video_len": 1}]


def test_config_keys_and_from_config():
    cfg = get_cfg()
    assert cfg.MODEL.MASK_FORMER.TEST.SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE is False
    assert cfg.MODEL.UniVS.TEST.DISABLE_SEMANTIC_QUERIES is False
    assert cfg.INPUT.LSJ_AUG.SQUARE_ENABLED is True and cfg.INPUT.LSJ_AUG.IMAGE_SIZE == 1024 and cfg.TEST.DETECTIONS_PER_IMAGE == 100
    cfg.MODEL.MASK_FORMER.TEST.PANOPTIC_ON = True
    cfg.MODEL.MASK_FORMER.TEST.OVERLAP_THRESHOLD = 0.8
    cfg.MODEL.UniVS.TEST.DISABLE_SEMANTIC_QUERIES = True
    d = InferenceImageGenericSegmentation(cfg, thing_contiguous_ids=range(80))
    assert d.panoptic_on and d.semantic_on and not d.instance_on and d.overlap_threshold == 0.8 and d.disable_semantic_queries
    assert d.LSJ_aug_enable_test and d.LSJ_aug_image_size == 1024 and d.test_topk_per_image == 100 and d.prompt_as_queries
    assert d.num_queries == 200 and d.thing_contiguous_ids == list(range(80))
    assert d.padded_size([(480, 640)]) == (1024, 1024)
    d.LSJ_aug_enable_test = False
    assert d.padded_size([(480, 641)]) == (480, 672)


def test_dispatch_reaches_the_image_driver_and_unknown_names_stay_loud():
    from univs_amd.modeling.meta_arch.univs_prompt import UniVS_Prompt_LongVideo
    model = build_model(image_cfg()).eval()
    seen = []
    real_eval = model.inference_img_generic_seg.eval
    model.inference_img_generic_seg.eval = lambda m, b: seen.append(b[0]["dataset_name"]) or ["ok"]
    assert model(image_input("coco_panoptic")) == ["ok"] and model(image_input("ade20k")) == ["ok"]
    assert seen == ["coco_panoptic", "ade20k"]
    model.inference_img_generic_seg.eval = real_eval
    for name in ("coco_2017_val", "ade20k_sem_seg_val"):            # not a vocabulary: raised before any device work
        with pytest.raises(NotImplementedError, match="vocabulary"):
            model(image_input(name))
    model.__class__ = UniVS_Prompt_LongVideo
    with pytest.raises(ValueError):
        model(image_input("coco_panoptic"))


def brute_force_nms(boxes, scores, labels, thr):
    """Greedy NMS written from its definition: visit by descending score (ties: lower index first), keep a box unless an already kept
    box of the same label overlaps it with IoU > thr (float64 areas of the inclusive-index corners as given)."""
    b = boxes.double().numpy()
    order = sorted(range(len(b)), key=lambda i: (-float(scores[i]), i))
    kept = []
    for i in order:
        ok = True
        for j in kept:
            if int(labels[i]) != int(labels[j]):
                continue
            iw = max(0.0, min(b[i, 2], b[j, 2]) - max(b[i, 0], b[j, 0]))
            ih = max(0.0, min(b[i, 3], b[j, 3]) - max(b[i, 1], b[j, 1]))
            inter = iw * ih
            ai = (b[i, 2] - b[i, 0]) * (b[i, 3] - b[i, 1])
            aj = (b[j, 2] - b[j, 0]) * (b[j, 3] - b[j, 1])
            if inter / (ai + aj - inter) > thr:
                ok = False
                break
        if ok:
            kept.append(i)
    return kept


@pytest.mark.parametrize("seed", range(6))
def test_batched_nms_matches_the_greedy_definition(seed):
    g = torch.Generator().manual_seed(seed)
    n = 60
    xy = torch.randint(0, 40, (n, 2), generator=g)
    wh = torch.randint(1, 25, (n, 2), generator=g)
    boxes = torch.cat([xy, xy + wh], 1).float()
    boxes[5] = boxes[4]                                            # identical boxes, equal scores: the lower index survives
    scores = torch.randint(0, 8, (n,), generator=g).float() / 8    # many ties
    labels = torch.randint(0, 3, (n,), generator=g)
    for thr in (0.3, 0.85, 0.9):
        got = batched_nms(boxes, scores, labels, thr).tolist()
        assert got == brute_force_nms(boxes, scores, labels, thr), thr
    assert nms(boxes[:0], scores[:0], 0.5).numel() == 0 and batched_nms(boxes[:0], scores[:0], labels[:0], 0.5).numel() == 0


def paint_like_the_reference(cur_masks, cur_scores, cur_classes, thing_ids, overlap):
    """panoptic_inference's loop (inference_image_generic_seg.py:330-379) over explicit masks: argmax, three sums per k, paint."""
    prob = cur_scores.view(-1, 1, 1) * cur_masks
    ids = prob.argmax(0)
    seg = torch.zeros(ids.shape, dtype=torch.int32)
    info, stuff, cur = [], {}, 0
    for k in range(cur_masks.shape[0]):
        c = int(cur_classes[k])
        isthing = c in thing_ids
        mask_area = int((ids == k).sum())
        original_area = int((cur_masks[k] >= 0.5).sum())
        mask = (ids == k) & (cur_masks[k] >= 0.5)
        if mask_area > 0 and original_area > 0 and int(mask.sum()) > 0:
            if mask_area / original_area < overlap:
                continue
            if not isthing:
                if c in stuff:
                    seg[mask] = stuff[c]
                    continue
                stuff[c] = cur + 1
            cur += 1
            seg[mask] = cur
            info.append({"id": cur, "isthing": bool(isthing), "category_id": c})
    return seg, info


@pytest.mark.parametrize("seed,overlap", [(0, 0.8), (1, 0.5), (2, 0.0)])
def test_panoptic_segment_table_matches_the_painting_loop(seed, overlap):
    L, _ = image_blob_logits(100 + seed, 40, 24, 32, 10)
    g = torch.Generator().manual_seed(seed)
    scores = torch.rand(40, generator=g)
    classes = torch.randint(0, 5, (40,), generator=g)              # repeated stuff classes: merges happen
    thing_ids = {0}
    steps = AtenSteps(L, (48, 64), (40, 60))
    planes = torch.arange(40)
    ids, counts = steps.panoptic_ids(planes, scores)
    lut, info = panoptic_segments(counts.numpy(), classes.numpy(), thing_ids, overlap)
    pan, seen = AtenSteps.panoptic_paint(ids, lut, (40, 60))
    ref, ref_info = paint_like_the_reference(steps.cropped(planes).sigmoid(), scores, classes, thing_ids, overlap)
    assert torch.equal(pan, ref) and info == ref_info
    if overlap == 0.0:                                             # a stuff merge took place
        assert any(not i["isthing"] for i in info) and len(set(lut) - {0}) < sum(1 for v in lut if v)
    present = {lut[k] for k in range(len(lut)) if seen[k]}
    assert present == set(torch.unique(ref).tolist()) - {0}


@pytest.mark.parametrize("n_in,n_out", [(40, 60), (60, 40), (37, 101), (101, 37), (64, 64), (32, 64), (768, 480), (683, 427)])
def test_nearest_index_rule_matches_interpolate(n_in, n_out):
    x = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
    ref = F.interpolate(x, size=(n_out, 1), mode="nearest")[0, 0, :, 0].long().numpy()
    assert np.array_equal(nearest_source_index(np.arange(n_out), n_in, n_out), ref)


def test_coco_panoptic_image_end_to_end_returns_all_three_results():
    cfg = image_cfg(SEMANTIC_ON=True, INSTANCE_ON=True, PANOPTIC_ON=True)
    model = build_model(cfg).eval()
    synth.load_synthetic(model)
    model.inference_img_generic_seg.thing_contiguous_ids = list(range(80))
    with cpu_ops():
        out = model(image_input("coco_panoptic"))
    assert len(out) == 1
    r = out[0]
    assert r["sem_seg"].shape == (133, 60, 75) and r["sem_seg"].dtype == torch.float32
    pan, info = r["panoptic_seg"]
    assert pan.shape == (60, 75) and pan.dtype == torch.int32
    assert set(torch.unique(pan).tolist()) - {0} == {i["id"] for i in info}
    inst = r["instances"]
    assert inst.image_size == (60, 75) and inst.pred_masks.shape == (len(inst.scores), 60, 75) and inst.pred_boxes.tensor.shape == (len(inst.scores), 4)
    assert len(inst.scores) == 100 and int(inst.pred_classes.max()) < 80
    assert len(r["instances_rle"]) == 100 and all(rle["size"] == [60, 75] for rle in r["instances_rle"])


def test_panoptic_and_instance_refuse_to_run_without_thing_categories():
    """Without thing categories every COCO thing would silently become stuff (same-class instances merged): loud instead.  A mapping
    gives each vocabulary its own list."""
    L, cls = image_blob_logits(5, 60, 16, 16, 133, (12, 16))
    d = InferenceImageGenericSegmentation(image_cfg(PANOPTIC_ON=True, SEMANTIC_ON=False))
    with pytest.raises(ValueError, match="thing"):
        d.postprocess(cls, L, (64, 64), (48, 64), (48, 64), dataset_name="coco_panoptic")
    with pytest.raises(ValueError, match="thing"):
        d.eval(None, image_input("coco_panoptic"))                 # before any model or device work
    d.thing_contiguous_ids = {"ade20k": list(range(150))}
    assert d.things("ade20k") == list(range(150)) and d.things("coco_panoptic") == []
    with pytest.raises(ValueError, match="thing"):
        d.postprocess(cls, L, (64, 64), (48, 64), (48, 64), dataset_name="coco_panoptic")
    d.thing_contiguous_ids = {"coco_panoptic": list(range(80))}
    pan, info = d.postprocess(cls, L, (64, 64), (48, 64), (48, 64), dataset_name="coco_panoptic")["panoptic_seg"]
    assert pan.shape == (48, 64)
    d.panoptic_on = False                                           # semantic alone needs no thing categories
    d.semantic_on = True
    d.thing_contiguous_ids = ()
    assert d.postprocess(cls, L, (64, 64), (48, 64), (48, 64))["sem_seg"].shape == (133, 48, 64)

