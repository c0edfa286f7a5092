"""Per-image evaluation at the shipped geometry: one COCO-panoptic image under the 1024 x 1024 LSJ square (a 768 x 1024 image of a
480 x 640 original), Swin-T, Q' = 200 learnable + 133 text queries, semantic + panoptic + instance results.  Prints one JSON line:

  model_ms            backbone + pixel decoder + decoder (the model's forward at T = 1, synthetic weights); `model_queries` says how
                      many queries that forward made: the reference's targets for a 'detection' image carry visual prompts, so the
                      model runs its 200 learnable queries only, while the post-processing runs on Q' = 333 (`post_queries`)
  post_fused_ms       InferenceImageGenericSegmentation.postprocess on csrc/image_post.hip
  post_aten_ms        the same driver on the ATen formulation of the same steps (the reference's expressions, the resized stack built)
  *_bytes             algorithmic bytes each path moves (see `bytes_moved`)
  fused_roofline      the fused path's bytes / time over the 8 TB/s HBM peak

Post-processing runs on closed-form logits (workloads.image_blob_logits: segments, overlaps and stuff merges actually happen); the
model's own logits under synthetic weights make few masks.  Each figure: `--warmup` untimed runs, then `--samples` timed ones (CUDA
events around a synchronised call); median, min and max are reported.

    python tools/image_bench.py [--samples 10] [--warmup 3] [--no-model]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from univs_amd.config import get_cfg                                   # noqa: E402
from univs_amd.inference.image_generic_seg import InferenceImageGenericSegmentation   # noqa: E402
from univs_amd.workloads import clip_table, image_blob_logits            # noqa: E402

Q_LEARN, C, HP, CROP, ORIG, LOWRES = 200, 133, 1024, (768, 1024), (480, 640), 256


def timed(fn, warmup, samples):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3), "n": samples}


def cfg_image():
    cfg = get_cfg()
    cfg.INPUT.SAMPLING_FRAME_NUM = 1
    cfg.MODEL.UniVS.CLIP_CLASS_EMBED_PATH = clip_table()
    cfg.MODEL.UniVS.LANGUAGE_ENCODER_ENABLE = False
    for k in ("SEMANTIC_ON", "INSTANCE_ON", "PANOPTIC_ON"):
        cfg.MODEL.MASK_FORMER.TEST[k] = True
    cfg.MODEL.MASK_FORMER.TEST.OVERLAP_THRESHOLD = 0.8
    cfg.MODEL.MASK_FORMER.TEST.OBJECT_MASK_THRESHOLD = 0.05
    return cfg


def bytes_moved(Qp, kept_pan, kept_inst):
    """Algorithmic bytes.  Fused: the logits once per kernel that reads all of them (stats), the kept planes once per kernel that reads
    them (panoptic ids, semseg: 200, instance masks: kept_inst), the outputs (ids, the painted map, R [C, crop] written and read by the
    resize, sem_seg, the instance masks).  ATen: the [Q', Hp, Wp] stack written once and read by the counts (2 passes), the crop's
    sigmoid / product / argmax / per-segment passes over the kept planes, the semantic einsum's sigmoid planes, the second resize of the
    kept instances, the same outputs."""
    lowres = LOWRES * LOWRES * 4
    crop = CROP[0] * CROP[1]
    orig = ORIG[0] * ORIG[1]
    outputs = crop * 4 + orig * 4 + 2 * C * crop * 4 + C * orig * 4 + kept_inst * orig
    fused = Qp * lowres + (kept_pan + 200 + kept_inst) * lowres + outputs
    stack = Qp * HP * HP * 4
    aten = (Qp * lowres + stack + 2 * stack                      # resize, the two quality counts
            + kept_pan * crop * 4 * 4 + kept_pan * crop * 4      # sigmoid, product, argmax, the per-segment sums
            + 200 * crop * 4 * 2                                 # semantic sigmoid planes (write + read)
            + kept_inst * crop * 4 + kept_inst * orig * 4        # second resize of the kept instances
            + outputs)
    return fused, aten


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.backends.cuda.matmul.allow_tf32 = False
    out = {"geometry": {"padded": [HP, HP], "crop": list(CROP), "original": list(ORIG), "queries": Q_LEARN + C, "lowres": [LOWRES, LOWRES],
                        "backbone": "Swin-T"}, "device": torch.cuda.get_device_name(0)}
    cfg = cfg_image()
    with torch.no_grad():
        if not args.no_model:
            from univs_amd import synth
            from univs_amd.modeling.build import build_model
            model = build_model(cfg).eval().to(dev)
            synth.load_synthetic(model)
            model.to(dev)
            frame = synth.synthetic_frames(1, CROP[0], CROP[1], "image_bench/frame")[0].to(dev)
            drv = model.inference_img_generic_seg
            inp = [{"image": [frame], "height": ORIG[0], "width": ORIG[1], "task": "detection", "dataset_name": "coco_panoptic",
                    "file_names": ["bench.jpg"], "video_len": 1}]
            images = drv.image_list([frame])
            targets = model.prepare_targets.process_inference(inp, tuple(images.tensor.shape[-2:]), dev, model.text_prompt_encoder,
                                                              images.image_sizes[0])
            head_out = {}

            def run_model():
                head_out["o"] = model.sem_seg_head(model.backbone(images.tensor), targets=targets)

            out["model_ms"] = timed(run_model, args.warmup, args.samples)
            pm = head_out["o"]["pred_masks"]
            out["model_pred_masks_shape"] = list(pm.shape)
            out["model_queries"] = int(pm.shape[1])
        L, cls = image_blob_logits(2024, Q_LEARN + C, LOWRES, LOWRES, C, (CROP[0] * LOWRES // HP, CROP[1] * LOWRES // HP))
        L, cls = L.to(dev), cls.to(dev)
        out["post_queries"] = int(L.shape[0])
        fused = InferenceImageGenericSegmentation(cfg, thing_contiguous_ids=range(80))
        aten = InferenceImageGenericSegmentation(cfg, thing_contiguous_ids=range(80))
        aten.fused = False
        res = {}

        def run(d, key):
            res[key] = d.postprocess(cls, L, (HP, HP), CROP, ORIG)

        out["post_fused_ms"] = timed(lambda: run(fused, "f"), args.warmup, args.samples)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run(fused, "f")
        torch.cuda.synchronize()
        out["post_fused_peak_bytes"] = torch.cuda.max_memory_allocated() - base
        out["post_aten_ms"] = timed(lambda: run(aten, "a"), args.warmup, args.samples)
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run(aten, "a")
        torch.cuda.synchronize()
        out["post_aten_peak_bytes"] = torch.cuda.max_memory_allocated() - base
    r = res["f"]
    kept_inst = len(r["instances"].scores)
    kept_pan = len(r["panoptic_seg"][1])
    fb, ab = bytes_moved(Q_LEARN + C, kept_pan, kept_inst)
    out.update({"segments": kept_pan, "instances": kept_inst, "fused_bytes": fb, "aten_bytes": ab,
                "speedup_post": round(out["post_aten_ms"]["median"] / out["post_fused_ms"]["median"], 2),
                "fused_roofline": round(fb / (out["post_fused_ms"]["median"] * 1e-3) / 8e12, 4),
                "segments_equal": r["panoptic_seg"][1] == res["a"]["panoptic_seg"][1]})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
