"""CPU: the MinVIS-style drivers of the non-unified configs (univs_amd/inference/video_minvis.py) -- config keys, the non-unified dispatch
of `UniVS_Prompt` / `UniVS_Prompt_LongVideo`, the running-sum mean against the reference's stack-and-mean, both drivers on their ATen
formulation against the reference's results (golden g24_*, tools/gen_golden_minvis.py), the COCO-json conversion, and both shipped
configs' inference keys end to end through the model on the oracle's CPU operators."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import c_ops
from oracle.cpu_path import cpu_ops
from tests import cases
from univs_amd import synth
from univs_amd.config import get_cfg
from univs_amd.inference.results import write_vps_predictions
from univs_amd.inference.video_minvis import (InferenceVideoVISFast, InferenceVideoVPS, clip_frame_counts, instances_to_coco_json_video,
                                              scale_to_mean_)
from univs_amd.modeling.build import build_model
from univs_amd.workloads import MinVISClipHead

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOTAL_CLASSES = 3938


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {k: g[k] for k in g.files}, json.loads(bytes(g["recipe"]).decode())


def stand_ins(r):
    head = MinVISClipHead(r["seed"], r["V"], r["Q"], r["h"], r["w"], TOTAL_CLASSES, r["start"], r["C"], r["n_obj"], extra=r["extra"],
                          classes=r.get("classes"))
    model = type("M", (), {})()
    model.backbone = lambda x: {"res2": x}
    model.sem_seg_head = head
    Hp, Wp = r["padded"]
    images = type("I", (), {})()
    images.tensor = torch.zeros(r["V"], 1, Hp, Wp)
    images.image_sizes = [tuple(r["crop"])] * r["V"]
    inputs = [{"dataset_name": r["dataset"], "height": r["out"][0], "width": r["out"][1], "video_id": 7, "video_len": r["V"]}]
    return model, inputs, images, [{}]


def driver(r, device="cpu", fused=True):
    common = dict(num_queries=r["num_queries"], stability_score_thresh=r["stability"], size_divisibility=32, LSJ_aug_image_size=1024,
                  LSJ_aug_enable_test=False, pixel_mean=[0.0] * 3, pixel_std=[1.0] * 3, num_frames=r["T"], num_frames_window_test=r["window"],
                  test_topk_per_image=r["topk"], fused=fused)
    if r["task"] == "vis":
        d = InferenceVideoVISFast(zero_shot_inference=r["zero_shot"], **common)
    else:
        d = InferenceVideoVPS(object_mask_threshold=r["object_mask"], overlap_threshold=r["overlap"],
                              thing_dataset_ids=r["things"], **common)
    return d.to(device)


def run_driver(r, device="cpu", fused=True):
    model, inputs, images, targets = stand_ins(r)
    images.tensor = images.tensor.to(device)
    head = model.sem_seg_head
    model.sem_seg_head = lambda f, targets=None: {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in head(f, targets).items()}
    d = driver(r, device, fused)
    with torch.no_grad():
        if r["task"] == "vis":
            return d.inference_video_vis_minvis(model, inputs, images, targets)
        return d.inference_video_vps_online(model, inputs, images, targets)


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape).astype(bool)


def check_vis(res, g, r, exact):
    """Records compared as a set keyed by (row, label): the row is identified by its masks.  Masks may differ only at recorded
    near-zero logits (none at all when `exact`)."""
    n = int(g["n"])
    V, (H0, W0) = r["V"], r["out"]
    ref_masks = unpack(g["masks"], (n, V, H0, W0))
    near0 = unpack(g["near0"], (n, V, H0, W0))
    assert res["image_size"] == tuple(r["out"]) and len(res["pred_scores"]) == n == len(res["pred_labels"]) == len(res["pred_masks"])
    got = {}
    for s, l, m in zip(res["pred_scores"], res["pred_labels"], res["pred_masks"]):
        assert m.dtype == torch.bool and tuple(m.shape) == (V, H0, W0) and m.device.type == "cpu"
        got.setdefault(int(l), []).append((float(s), m.numpy()))
    assert sorted(res["pred_scores"], reverse=True) == list(res["pred_scores"])      # the documented order
    for i in range(n):
        cands = got[int(g["labels"][i])]
        ok = [j for j, (s, m) in enumerate(cands)
              if abs(s - float(g["scores"][i])) <= (0 if exact else 1e-5 * max(1.0, abs(float(g["scores"][i]))))
              and ((m == ref_masks[i]) | near0[i]).all()]
        assert ok, (i, g["labels"][i], g["scores"][i], [s for s, _ in cands])
        cands.pop(ok[0])


def check_vps(res, g, r, exact):
    pan = res["pred_masks"]
    assert pan.dtype == torch.int32 and pan.device.type == "cpu" and res["task"] == "vps"
    out = tuple(int(v) for v in g["out_size"])
    assert res["image_size"] == out and tuple(pan.shape) == (r["V"],) + out
    tie = unpack(g["pan_tie"], tuple(pan.shape))
    diff = pan.numpy() != g["pan"].astype(np.int32)
    assert not (diff & ~tie).any(), int((diff & ~tie).sum())
    if exact:
        assert not diff.any()
    assert res["segments_infos"] == json.loads(bytes(g["segments_infos"]).decode())
    assert [int(v) for v in res["pred_ids"]] == g["pred_ids"].tolist()


# ---- config and dispatch ------------------------------------------------------------------------------------------------------------
def test_config_defaults_and_from_config():
    cfg = get_cfg()
    t = cfg.MODEL.BoxVIS.TEST
    assert t.TRACKER_TYPE == "minvis" and t.ZERO_SHOT_INFERENCE is False and t.WINDOW_INFERENCE is False and t.MERGE_ON_CPU is False
    cfg.MODEL.BoxVIS.TEST.ZERO_SHOT_INFERENCE = True
    cfg.MODEL.BoxVIS.TEST.MERGE_ON_CPU = True
    cfg.MODEL.MASK_FORMER.TEST.OBJECT_MASK_THRESHOLD = 0.05
    vis, vps = InferenceVideoVISFast(cfg), InferenceVideoVPS(cfg, thing_dataset_ids=[1, 2])
    assert vis.zero_shot_inference and vis.merge_on_cpu and vis.tracker_type == "minvis" and vis.num_frames_window_test == 5
    assert vis.num_queries == 200 and vis.test_topk_per_image == 100 and vis.LSJ_aug_enable_test
    assert vps.object_mask_threshold == 0.05 and vps.thing_dataset_ids == [1, 2] and vps.change_to_720p


def nonunified_model(meta="UniVS_Prompt", **box):
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE = meta
    cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES = 20
    cfg.MODEL.UniVS.CLIP_CLASS_EMBED_PATH = cases.clip_table()
    cfg.MODEL.UniVS.TEST.VIDEO_UNIFIED_INFERENCE_ENABLE = False
    for k, v in box.items():
        cfg.MODEL.BoxVIS.TEST[k] = v
    return build_model(cfg).eval()


def video_input(dataset, n=4, H=64, W=96, task="detection", **extra):
    d = {"image": list(synth.synthetic_frames(n, H, W, "minvis/frames")), "video_len": n, "height": H, "width": W, "task": task,
         "dataset_name": dataset, "file_names": [f"videos/v0/{i:05d}.jpg" for i in range(n)], "video_id": 3}
    d.update(extra)
    return [d]


@pytest.mark.parametrize("meta", ["UniVS_Prompt", "UniVS_Prompt_LongVideo"])
def test_non_unified_dispatch(meta):
    model = nonunified_model(meta)
    seen = []
    model.inference_video_vis_fast.eval = lambda m, b: seen.append(("vis", b[0]["dataset_name"])) or {"vis": 1}
    model.inference_video_vps.eval = lambda m, b: seen.append(("vps", b[0]["dataset_name"])) or {"vps": 1}
    model.inference_video_vos.eval = lambda m, b: seen.append(("vos", b[0]["dataset_name"])) or ["vos"]
    for name in ("ytvis21", "ovis", "ytvis_2019_val"):
        assert model(video_input(name)) == {"vis": 1}
    for name in ("vipseg", "vpsw_dev"):
        assert model(video_input(name)) == {"vps": 1}
    assert seen[:5] == [("vis", "ytvis21"), ("vis", "ovis"), ("vis", "ytvis_2019_val"), ("vps", "vipseg"), ("vps", "vpsw_dev")]
    with pytest.raises(ValueError, match="Not support"):
        model(video_input("kitti_step"))
    if meta == "UniVS_Prompt_LongVideo":
        assert model(video_input("sot_davis")) == ["vos"]
    else:
        with pytest.raises(ValueError, match="Not support"):
            model(video_input("sot_davis"))
    model.tracker_type = "mdqe"
    with pytest.raises(NotImplementedError, match="TRACKER_TYPE 'mdqe'"):
        model(video_input("ovis"))


def test_drivers_check_the_vocabulary_before_any_model_call():
    model = nonunified_model()
    for name, d in (("ytvis_2021", "inference_video_vis_fast"), ("vipseg_panoptic_val", "inference_video_vps")):
        with pytest.raises(NotImplementedError, match="vocabulary"):
            model(video_input(name))
    with pytest.raises(ValueError, match="vspw"):
        model.inference_video_vps.eval(None, video_input("vspw"))                   # a vocabulary, but not a VPS dataset
    model.inference_video_vps.thing_dataset_ids = []
    with pytest.raises(ValueError, match="thing"):
        model.inference_video_vps.eval(None, video_input("vipseg"))
    with pytest.raises(NotImplementedError, match="frame sharding"):
        model.inference_video_vis_fast.set_frame_shard(object())
    model.inference_video_vis_fast.frame_shard = object()
    with pytest.raises(NotImplementedError, match="frame sharding"):
        model.inference_video_vis_fast.eval(None, video_input("ovis"))


def test_direct_construction_keeps_working_without_the_drivers():
    from univs_amd.modeling.meta_arch.univs_prompt import UniVS_Prompt
    m = nonunified_model()
    bare = UniVS_Prompt(backbone=m.backbone, sem_seg_head=m.sem_seg_head, prepare_targets=m.prepare_targets, text_prompt_encoder=None,
                        inference_video_entity=m.inference_video_entity, inference_video_vos=m.inference_video_vos,
                        pixel_mean=[0, 0, 0], pixel_std=[1, 1, 1], video_unified_inference_enable=False, custom_videos_enable=False,
                        custom_videos_text=[]).eval()
    with pytest.raises(NotImplementedError, match="inference_video_vis_fast"):
        bare(video_input("ovis"))


# ---- the running-sum mean ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n_clips", [(2, 8), (3, 7), (1, 5), (4, 2)])
def test_running_sum_mean_matches_the_stack_and_mean(T, n_clips):
    """The reference's stack-and-mean (vis_fast :278-293) against the running sum scaled in place: bit-identical at T <= 2, within
    the rounding of the summation order otherwise."""
    g = torch.Generator().manual_seed(T * 100 + n_clips)
    clips = [torch.randn(5, T, 6, 7, generator=g) * 4 for _ in range(n_clips)]
    ref = []
    for v in range(n_clips + T - 1):
        m = [clips[v - t][:, t] for t in range(min(v + 1, T)) if v - t < n_clips]
        ref.append(torch.stack(m).mean(dim=0))
    ref = torch.stack(ref, dim=1)
    S = torch.zeros(5, n_clips + T - 1, 6, 7)
    for i, c in enumerate(clips):
        S[:, i:i + T] += c
    got = scale_to_mean_(S, clip_frame_counts(n_clips, T))
    if T <= 2:
        assert torch.equal(got, ref)
    else:
        torch.testing.assert_close(got, ref, rtol=1e-6, atol=1e-6)


# ---- both drivers against the reference's results ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g24_vis_t2", "g24_vis_t3", "g24_vis_zero_shot"])
def test_vis_driver_cpu_matches_reference(name):
    g, r = load_golden(name)
    check_vis(run_driver(r), g, r, exact=r["T"] == 2)


@pytest.mark.parametrize("name", ["g24_vps_t2", "g24_vps_t3"])
def test_vps_driver_cpu_matches_reference(name):
    g, r = load_golden(name)
    check_vps(run_driver(r), g, r, exact=r["T"] == 2)


def test_vps_keep_rule_names_both_settings_when_rows_are_short():
    g, r = load_golden("g24_vps_t2")
    r = dict(r, topk=50)
    with pytest.raises(ValueError, match="DETECTIONS_PER_IMAGE.*OBJECT_MASK_THRESHOLD"):
        run_driver(r)


def test_coco_json_video_matches_oracle_rle():
    g, r = load_golden("g24_vis_t2")
    res = run_driver(r)
    inputs = [{"video_id": 7, "height": r["out"][0], "width": r["out"][1]}]
    js = instances_to_coco_json_video(inputs, res)
    assert len(js) == len(res["pred_scores"])
    for rec, s, l, m in zip(js, res["pred_scores"], res["pred_labels"], res["pred_masks"]):
        assert rec["video_id"] == 7 and rec["score"] == s and rec["category_id"] == l and (rec["height"], rec["width"]) == tuple(r["out"])
        assert len(rec["segmentations"]) == r["V"]
        for seg, frame in zip(rec["segmentations"], m.numpy()):
            assert seg == {"size": list(r["out"]), "counts": c_ops.rle_encode(frame)[1]}


# ---- the shipped configs' inference keys end to end ----------------------------------------------------------------------------------
def shipped_cfg(vps):
    cfg = get_cfg()
    cfg.MODEL.META_ARCHITECTURE = "UniVS_Prompt"
    cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES = 20
    cfg.MODEL.UniVS.CLIP_CLASS_EMBED_PATH = cases.clip_table()
    cfg.MODEL.UniVS.TEST.VIDEO_UNIFIED_INFERENCE_ENABLE = False
    cfg.MODEL.BoxVIS.TEST.TRACKER_TYPE = "minvis"
    cfg.MODEL.BoxVIS.TEST.NUM_FRAMES_WINDOW = 1 if vps else 5
    cfg.INPUT.SAMPLING_FRAME_NUM = 2
    cfg.INPUT.LSJ_AUG.IMAGE_SIZE = 128
    cfg.MODEL.MASK_FORMER.TEST.OVERLAP_THRESHOLD = 0.8
    cfg.MODEL.MASK_FORMER.TEST.OBJECT_MASK_THRESHOLD = 0.05 if vps else 0.1
    cfg.TEST.DETECTIONS_PER_IMAGE = 10 if vps else 100
    return cfg


def test_shipped_vis_config_returns_the_reference_dict():
    model = build_model(shipped_cfg(False)).eval()
    synth.load_synthetic(model)
    with cpu_ops():
        out = model(video_input("ovis", n=4))
    assert set(out) == {"image_size", "pred_scores", "pred_labels", "pred_masks"} and out["image_size"] == (64, 96)
    assert len(out["pred_scores"]) == len(out["pred_labels"]) == len(out["pred_masks"]) >= 5
    assert all(isinstance(s, float) for s in out["pred_scores"]) and all(0 <= l < 25 for l in out["pred_labels"])
    assert all(m.dtype == torch.bool and tuple(m.shape) == (4, 64, 96) for m in out["pred_masks"])


def test_shipped_vps_config_output_feeds_write_vps_predictions(tmp_path):
    model = build_model(shipped_cfg(True)).eval()
    synth.load_synthetic(model)
    model.inference_video_vps.thing_dataset_ids = list(range(1, 59))
    inp = video_input("vipseg", n=3, frame_indices=[0, 1, 2])
    with cpu_ops():
        out = model(inp)
    assert set(out) == {"image_size", "pred_masks", "segments_infos", "pred_ids", "task"} and out["task"] == "vps"
    assert out["image_size"] == (720, 1080) and out["pred_masks"].shape == (3, 720, 1080) and out["pred_masks"].dtype == torch.int32
    categories = {c: {"id": c, "isthing": int(c <= 58), "color": [c, 255 - c, (7 * c) % 256]} for c in range(1, 125)}
    rec = write_vps_predictions(inp[0], out, str(tmp_path), categories)
    assert rec["video_id"] == "v0" and len(rec["annotations"]) == 3
    assert len(os.listdir(tmp_path / "pan_pred" / "v0")) == 3
