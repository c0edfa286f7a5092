"""`python -m univs_amd.run`: a checkpoint and frames on disk to result files.

    python -m univs_amd.run --config-file F --weights W (--json J --image-root R --dataset-name N | --video-dir D) --output-dir O
                            [--masks-dir A --dataset-name N [--vos-meta M]]
                            [--resize gpu|host] [--decode host|gpu] [--png host|gpu] [--reader host|gpu]
                            [--visualize off|host|gpu [--categories-json C]]
                            [--gt-json G [--hota] | --pan-gt-json P --truth-dir T | --davis-root V | --pvos-data V]
                            [KEY VALUE ...]
    python -m univs_amd.run --config-file F --weights W (--image-dir D | --pan-gt-json P --image-root R --truth-dir T [--sem-gt-dir S]) [--inst-gt-json G]
                            --dataset-name coco_panoptic|coco|ade20k --output-dir O [--categories-json C] [--batch B] ...

The model is `build_model(load_cfg(F, [KEY VALUE ...]))` with `ckpt["model"]` loaded strictly (the reference's state-dict layout).  The
frames are the videos of a YouTube-VIS-format file, or the sub-folders of a folder of jpg / png frames (data/datasets.py), mapped by
data.VideoTestMapper.  With --gt-json the outputs go to evaluation.YTVISEvaluator (results.json; AP / AR when the file has annotations),
or with --hota to evaluation.hota.HOTAEvaluator (results.json, hota-final.txt),
with --pan-gt-json and --truth-dir to evaluation.VPSEvaluator; without either each video's driver output is saved to O/<video_id>.pt.

A --dataset-name of a video-object-segmentation data set (sot_*, mots_mose*, mots_burst*, pvos_*) reads the file with
data.load_vos_json and maps it with data.VOSTestMapper, first-frame masks included.  The id maps the VOS driver returns per clip are
written as palette PNGs to O/inference/Annotations/<video>/<frame>.png (`write_vos_outputs`); --davis-root V (the DAVIS folder that
holds Annotations/ and ImageSets/) then scores them with evaluation.DAVISEvaluator in its semi-supervised task (davis-metrics.txt in
O/inference), --pvos-data V (the VIPOSeg split folder) with evaluation.PVOSEvaluator (pvos-ious.txt); without either only the PNGs are
written.
--video-dir JPEGImages --masks-dir Annotations --dataset-name N reads a VOS data set from the folders it ships as, without a converted
json: data.vos_records_from_dirs makes the records by the rule of N (sot_davis16*, sot_davis17*, mots_mose*, sot_ytbvos18*, pvos_viposeg*;
--vos-meta names the folder of meta.json / obj_class.json, by default the one above --masks-dir; --reader says who decodes and counts
the annotation PNGs) and the mapper makes the prompt masks from the PNGs' id maps (csrc/idmap_prompts.hip with --resize gpu).  Writing
and scoring go as for the json.

--png gpu has the result PNGs (the VOS id maps, the VPS panoptic maps) compressed on the device by csrc/png_deflate.hip instead of by
Pillow on a host core: the same paths and the same pixels, mode and palette, other (larger) files; the default is host.
--reader gpu has the VPS, DAVIS and VIPOSeg evaluators decode the PNGs they score on the device (csrc/png_inflate.hip) instead of with
Pillow: the same numbers; the default is host.
--decode gpu (with --resize gpu) has the mappers decode the JPEG frames on the device (csrc/jpeg_decode.hip) instead of with Pillow: the
same pixels; files the decoder does not cover are read on the host as before; the default is host.
--visualize host|gpu writes something a person can look at: per video O/inference/Overlays/<video>/<frame>.jpg, the result drawn over the
file's own pixels at their original size (inference/overlay_rule.py: the table's colour blended in by its alpha, a contour where the id
changes), and a legend.json of the ids drawn.  Drawn are the VOS driver's id maps in the video's palette, the `pred_masks` of a VSS or VPS
output in the category colours (--categories-json, else the default palette) and VIS results that carry per-frame masks; an output without
a per-pixel result at the output size prints one line and writes nothing.  host draws with numpy and encodes with Pillow, gpu does both
inside csrc/jpeg_encode.hip: the same files byte for byte; with --decode gpu the frames never leave the device.  The default is off.

Images: a --dataset-name of an image vocabulary (coco_panoptic, coco, ade20k) runs the per-image driver on the jpg / png files of
--image-dir, or on the images of a panoptic ground-truth file (--pan-gt-json P --image-root R --truth-dir T: data.load_panoptic_json),
mapped by data.ImageTestMapper, --batch images per model call.  The class table (dataset ids, names, which classes are things) is read
from P's own `categories`, without P from --categories-json; the driver's `thing_contiguous_ids` are set from it and its semantic result
is asked for as labels (`sem_seg_as = "labels"`: csrc/semseg_labels.hip).  Written are O/inference/panoptic/<stem>.png with
O/inference/predictions.json (the segments' classes), O/inference/sem_seg/<stem>.png and O/inference/coco_instances_results.json, for the sub-tasks the config enables.  With P and T the
panoptic results are scored by evaluation.image.PanopticEvaluator (PQ / SQ / RQ), with --sem-gt-dir S (class-id PNGs named after the
images) the semantic ones by SemSegEvaluator (mIoU); both dictionaries are printed as one.  With --inst-gt-json G (a COCO
instances json, polygons) the instance results are scored with evaluation.coco.COCOInstanceEvaluator: mask AP.  --visualize draws
the panoptic map, else the semantic labels, to O/inference/Overlays.

A vocabulary of one's own: --class-names F (a text file, one name per line, or a json with a `categories` list) with --video-dir or
--image-dir.  The table is made from the names by the model's own CLIP text tower, or by --clip-weights W where the config builds none
(univs_amd/vocabulary.py), and installed under --dataset-name (default custom; none of the named vocabularies): the frames of
--video-dir then run through the unified entity loop under --sub-task vis | vss | vps (default vis; vps needs `isthing` in a json), the
images of --image-dir through the per-image driver with the class table taken from the vocabulary.  O/inference/vocabulary.json maps
contiguous id to name; the names reach the overlays' legend.json.  No evaluator runs: no ground truth shares such a vocabulary.
Without --class-names every run parses, runs and writes as before.
"""
import argparse
import json
import os
import sys

import torch

from .config import load_cfg
from .data import (ImageTestMapper, VideoTestMapper, VOSTestMapper, image_records_from_dir, is_vos_name, load_categories_json, load_panoptic_json,
                   load_video_json, load_vos_json, video_records_from_dir, vos_records_from_dirs)
from .engine import inference_on_images, inference_on_videos
from .inference.results import write_vos_pngs
from .modeling.build import build_model


IMAGE_NAMES = ("coco_panoptic", "coco", "ade20k")                    # the per-image driver's vocabularies (image_generic_seg.py: check_dataset)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m univs_amd.run", description="video and image inference from files on disk")
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--weights", required=True, help="a checkpoint whose \"model\" entry is the state dict")
    ap.add_argument("--json", help="a YouTube-VIS-format test file")
    ap.add_argument("--image-root", help="the folder the file names of --json are relative to")
    ap.add_argument("--dataset-name", help="the registered name of --json's data set, e.g. ytvis_2021_val or sot_davis17_val")
    ap.add_argument("--video-dir", help="a folder whose sub-folders hold the frames of one video each")
    ap.add_argument("--masks-dir", help="with --video-dir and --dataset-name: the folder of the videos' annotation PNGs (a VOS data set's Annotations)")
    ap.add_argument("--vos-meta", help="with --masks-dir: the folder of meta.json / obj_class.json (default: the one above --masks-dir)")
    ap.add_argument("--image-dir", help="a folder of jpg / png images: the per-image driver (with --dataset-name coco_panoptic, coco or ade20k)")
    ap.add_argument("--sem-gt-dir", help="an image run: the folder of class-id PNGs named after the images, scored with SemSegEvaluator")
    ap.add_argument("--inst-gt-json", default=argparse.SUPPRESS,      # (absent from the namespace unless given: the other runs' namespaces stay theirs)
                    help="an image run: a COCO instances json (polygons), the instance results scored with COCOInstanceEvaluator")
    ap.add_argument("--batch", type=int, default=1, help="an image run: images per model call")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--resize", choices=("gpu", "host"), default="gpu")
    ap.add_argument("--decode", choices=("host", "gpu"), default="host", help="who decodes the JPEG frames: Pillow, or the HIP decoder (needs --resize gpu)")
    ap.add_argument("--png", choices=("host", "gpu"), default="host", help="who compresses the result PNGs: Pillow, or the HIP encoder")
    ap.add_argument("--reader", choices=("host", "gpu"), default="host", help="who decodes the PNGs the evaluators score: Pillow, or the HIP decoder")
    ap.add_argument("--visualize", choices=("off", "host", "gpu"), default="off",
                    help="write overlay JPEGs of the results: drawn and encoded by numpy and Pillow, or by the HIP encoder")
    ap.add_argument("--categories-json", help="with --visualize: a file whose \"categories\" ({id, name, color}) colour and name VPS / VSS classes")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--gt-json", help="YouTube-VIS annotation file: score with YTVISEvaluator")
    ap.add_argument("--hota", action="store_true", help="with --gt-json: score with HOTAEvaluator instead of YTVISEvaluator")
    ap.add_argument("--pan-gt-json", help="VIPSeg panoptic ground-truth json: score with VPSEvaluator (with --truth-dir)")
    ap.add_argument("--truth-dir", help="the folder of the ground-truth panoptic PNGs")
    ap.add_argument("--davis-root", help="the DAVIS folder (Annotations/, ImageSets/): score a sot_davis* run with DAVISEvaluator")
    ap.add_argument("--pvos-data", help="the VIPOSeg split folder (Annotations/, meta files): score a pvos_* run with PVOSEvaluator")
    ap.add_argument("--class-names", help="with --video-dir or --image-dir: the class vocabulary of the run, a text file (one name per line) or "
                                          "a json with a `categories` list; its table is made by the CLIP text tower (univs_amd/vocabulary.py)")
    ap.add_argument("--clip-weights", help="with --class-names: a converted CLIP text-tower checkpoint, where the config builds no language encoder")
    ap.add_argument("--sub-task", choices=("vis", "vss", "vps"), help="with --class-names and --video-dir: what the entity loop produces "
                                                                      "(default vis; vps needs `isthing`, i.e. a categories json)")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE pairs merged into the config")
    args = ap.parse_args(argv)
    from_json = args.json is not None
    check_class_name_args(ap, args)
    if args.image_dir is not None and (from_json or args.video_dir is not None):
        ap.error("--image-dir is a source of its own: not with --json or --video-dir")
    args.image = args.image_dir is not None or (not from_json and args.video_dir is None and args.dataset_name in IMAGE_NAMES and
                                                args.pan_gt_json is not None and args.image_root is not None)
    if args.image:
        return check_image_args(ap, args)
    if hasattr(args, "inst_gt_json"):
        ap.error("--inst-gt-json goes with an image run (--image-dir, or --pan-gt-json with --image-root and an image --dataset-name)")
    if args.sem_gt_dir is not None or args.batch != 1:
        ap.error("--sem-gt-dir and --batch go with an image run (--image-dir, or --pan-gt-json with --image-root and an image --dataset-name)")
    if from_json == (args.video_dir is not None):
        ap.error("give either --json (with --image-root and --dataset-name) or --video-dir")
    if from_json and not (args.image_root and args.dataset_name):
        ap.error("--json needs --image-root and --dataset-name")
    if args.masks_dir is not None and (from_json or not args.dataset_name):
        ap.error("--masks-dir goes with --video-dir and --dataset-name (a VOS data set in its folders), not with --json")
    if args.vos_meta is not None and args.masks_dir is None:
        ap.error("--vos-meta goes with --masks-dir")
    if (args.pan_gt_json is None) != (args.truth_dir is None):
        ap.error("--pan-gt-json and --truth-dir go together")
    if sum(v is not None for v in (args.gt_json, args.pan_gt_json, args.davis_root, args.pvos_data)) > 1:
        ap.error("one evaluator at a time: --gt-json, --pan-gt-json, --davis-root or --pvos-data")
    if args.hota and args.gt_json is None:
        ap.error("--hota scores against --gt-json")
    if args.masks_dir is not None and not is_vos_name(args.dataset_name):
        ap.error("--masks-dir reads a VOS data set (--dataset-name sot_*, mots_mose*, pvos_*)")
    args.vos = bool((from_json or args.masks_dir is not None) and is_vos_name(args.dataset_name))
    if (args.davis_root or args.pvos_data) and not args.vos:
        ap.error("--davis-root and --pvos-data score a VOS data set (--dataset-name sot_*, mots_mose*, mots_burst*, pvos_*)")
    if args.vos and (args.gt_json or args.pan_gt_json):
        ap.error("a VOS data set is scored with --davis-root or --pvos-data")
    if args.davis_root and not ("davis16" in args.dataset_name or "davis17" in args.dataset_name):
        ap.error("--davis-root needs a davis16 / davis17 --dataset-name")
    return args


def check_class_name_args(ap, args):
    """The rules of --class-names (a vocabulary made from names; without it nothing here applies)."""
    if args.class_names is None:
        if args.clip_weights is not None or args.sub_task is not None:
            ap.error("--clip-weights and --sub-task go with --class-names")
        return
    if args.json is not None:
        ap.error("--class-names goes with --video-dir or --image-dir, not with --json (a registered data set has its named vocabulary)")
    if args.masks_dir is not None:
        ap.error("--class-names is not for a VOS run (--masks-dir): it has no class vocabulary")
    if args.gt_json or args.pan_gt_json or args.sem_gt_dir or hasattr(args, "inst_gt_json") or args.davis_root or args.pvos_data:
        ap.error("--class-names: the ground truth of a registered data set does not share a vocabulary made from names; no evaluator")
    if args.image_dir is not None and args.sub_task is not None:
        ap.error("--sub-task chooses what the video entity loop produces; an image run has none")
    if args.dataset_name is None:
        args.dataset_name = "custom"
    if args.dataset_name in IMAGE_NAMES or is_vos_name(args.dataset_name):
        ap.error("--class-names installs a vocabulary of its own: --dataset-name names it and is none of the named ones (default custom)")
    if args.sub_task == "vps":
        from .vocabulary import read_names
        if not os.path.isfile(args.class_names) or read_names(args.class_names)[1] is None:
            ap.error("--sub-task vps needs to know which names are things: give --class-names a json whose categories carry `isthing`")


def check_image_args(ap, args):
    """The argument rules of an image run, in the style of the video ones."""
    if args.class_names is None and args.dataset_name not in IMAGE_NAMES:
        ap.error("an image run needs --dataset-name coco_panoptic, coco or ade20k (or --class-names)")
    if (args.pan_gt_json is None) != (args.truth_dir is None):
        ap.error("--pan-gt-json and --truth-dir go together")
    if args.image_dir is None and not args.image_root:
        ap.error("--pan-gt-json as the source of an image run needs --image-root")
    if args.class_names is None and args.pan_gt_json is None and args.categories_json is None:
        ap.error("an image run reads its class table from --pan-gt-json, or without one from --categories-json")
    if args.masks_dir is not None or args.vos_meta is not None or args.gt_json or args.hota or args.davis_root or args.pvos_data:
        ap.error("--masks-dir, --vos-meta, --gt-json, --hota, --davis-root and --pvos-data belong to video runs")
    if args.batch < 1:
        ap.error("--batch is at least 1")
    if hasattr(args, "inst_gt_json") and not os.path.isfile(args.inst_gt_json):
        ap.error(f"--inst-gt-json: {args.inst_gt_json} is not a file")
    args.vos = False
    return args


def build_image_evaluators(args, table, records):
    from .evaluation.image import PanopticEvaluator, SemSegEvaluator
    evaluators = []
    if args.pan_gt_json:
        evaluators.append(PanopticEvaluator(args.pan_gt_json, args.truth_dir, args.output_dir, class_table=table, device=args.device, png=args.png,
                                            reader=args.reader))
    if args.sem_gt_dir:
        evaluators.append(SemSegEvaluator(args.sem_gt_dir, len(table["ids"]), 255, table["names"], args.output_dir, device=args.device, png=args.png,
                                          reader=args.reader))
    return evaluators


def image_overlay_table(args, output, table):
    """(0, ids [1, H, W], lut, {row: name}) of one image's result: the panoptic map in its segments' category colours, else the
    semantic labels; a sentence where the output holds neither."""
    from .inference import overlay_rule as ov
    from .inference.results import semseg_labels_of
    source = argparse.Namespace(categories_json=args.categories_json or args.pan_gt_json)
    if source.categories_json is not None:                          # (None: a --class-names run without --categories-json)
        with open(source.categories_json) as f:
            if not all("color" in c for c in json.load(f)["categories"]):
                source.categories_json = None                       # no colours in the file: the default palette
    if "panoptic_seg" in output:
        pan, infos = output["panoptic_seg"]
        lut, names, rows = _category_table(source, ov.ALPHA_VPS, len(table["ids"]))
        ids = torch.zeros_like(pan, dtype=torch.int32)
        for info in infos:
            c = int(info["category_id"])
            ids[pan == int(info["id"])] = rows.get(table["ids"][c], 0) if rows is not None else c + 1
        return 0, ids[None], lut, names or {c + 1: n for c, n in enumerate(table["names"])}
    if "sem_seg_labels" in output or "sem_seg" in output:
        sem = semseg_labels_of(output).to(torch.int32)
        lut, names, rows = _category_table(source, ov.ALPHA_VSS, len(table["ids"]))
        if rows is not None:
            to_row = torch.tensor([rows.get(d, 0) for d in table["ids"]], dtype=torch.int32, device=sem.device)
            return 0, to_row[sem.long()][None], lut, names
        return 0, (sem + 1)[None], lut, {c + 1: n for c, n in enumerate(table["names"])}
    return "the output holds neither a panoptic map nor semantic labels"


def run_images(args, cfg, model):
    """An image run: records, class table, mapper, writers and evaluators around `inference_on_images`."""
    from .inference.results import image_instances_to_coco_json, write_instances_json, write_panoptic_prediction, write_semseg_prediction
    if getattr(args, "vocabulary", None) is not None:               # --class-names: the class table is the installed vocabulary's
        from .data.image_datasets import class_table
        vocab = args.vocabulary
        records = image_records_from_dir(args.image_dir)
        table = class_table([{"id": i, "name": n, "isthing": int(vocab.things is None or i in vocab.things)} for i, n in enumerate(vocab.names)])
    elif args.image_dir is not None:
        records = image_records_from_dir(args.image_dir)
        table = load_categories_json(args.pan_gt_json or args.categories_json)
    else:
        records, table = load_panoptic_json(args.pan_gt_json, args.image_root, args.truth_dir, semseg_dir=args.sem_gt_dir)
    for r in records:
        r["dataset_name"] = args.dataset_name
    driver = model.inference_img_generic_seg
    things = driver.thing_contiguous_ids if isinstance(driver.thing_contiguous_ids, dict) else {}
    things[args.dataset_name] = list(table["thing_contiguous_ids"])
    driver.thing_contiguous_ids = things
    driver.sem_seg_as = "labels"
    thing_dataset_ids = [table["ids"][c] for c in table["thing_contiguous_ids"]]      # an instance's class is its column among the things
    mapper = ImageTestMapper.from_config(cfg, resize=args.resize, device=args.device, decode=args.decode)
    os.makedirs(args.output_dir, exist_ok=True)
    evaluators = build_image_evaluators(args, table, records)
    writes_panoptic = any(type(ev).__name__ == "PanopticEvaluator" for ev in evaluators)
    instances, panoptic = [], []

    def on_output(inputs, outputs):
        for item, output in zip(inputs, outputs):
            if "panoptic_seg" in output and not writes_panoptic:
                panoptic.append(write_panoptic_prediction(item, output, args.output_dir, table["ids"], png=args.png))
            if "sem_seg_labels" in output or "sem_seg" in output:
                write_semseg_prediction(item, output, args.output_dir, table["ids"], png=args.png)
            if "instances" in output:
                instances.extend(image_instances_to_coco_json(item, output, thing_dataset_ids))
            if args.visualize != "off":
                write_image_overlay(args, item, output, table)
    results = inference_on_images(model, records, mapper, evaluators, on_output=on_output, batch=args.batch)
    if driver.instance_on:
        write_instances_json(instances, args.output_dir)
    if getattr(args, "inst_gt_json", None):
        results = score_instances(args, instances, results)
    if panoptic:                                                     # (the segments' classes: what PanopticEvaluator.evaluate writes when it runs)
        with open(os.path.join(args.output_dir, "inference", "predictions.json"), "w") as f:
            json.dump({"annotations": panoptic}, f)
    if evaluators or getattr(args, "inst_gt_json", None):
        print(json.dumps(results, default=str))
    return results


def score_instances(args, instances, results):
    """--inst-gt-json: mask AP of the instance records the run just wrote; the twelve summary lines are printed, the numbers join
    `results` under "segm"."""
    from .evaluation.coco import COCOInstanceEvaluator
    if not instances:
        print("--inst-gt-json: the run produced no instance records (the driver's instance output is off, or nothing was found); no mask AP")
        return results
    ev = COCOInstanceEvaluator(args.inst_gt_json, os.path.join(args.output_dir, "inference"), device=args.device)
    ev.process(instances)
    scores = ev.evaluate()
    for line in ev.last_eval.summary:
        print(line)
    results = dict(results) if results else {}
    results.update(scores)
    return results


def write_image_overlay(args, item, output, table):
    from .data import read_images
    from .inference.results import write_overlay_jpegs
    t = image_overlay_table(args, output, table)
    if isinstance(t, str):
        print(f"--visualize: image {item.get('image_id')}: {t}; nothing written")
        return []
    first, ids, lut, row_names = t
    names = item["file_names"][:1]
    frames = read_images(names, decode=args.decode, device=args.device if args.decode == "gpu" else None)
    paths = write_overlay_jpegs(args.output_dir, names, 0, frames, ids, lut, jpeg=args.visualize)
    present = torch.unique(torch.as_tensor(ids).long().clamp(0, len(lut) - 1)).tolist()
    with open(os.path.splitext(paths[0])[0] + ".legend.json", "w") as f:
        json.dump(_legend(lut, row_names, present), f, indent=1, sort_keys=True)
    return paths


def build_evaluator(args):
    if args.gt_json and getattr(args, "hota", False):
        from .evaluation.hota import HOTAEvaluator
        return HOTAEvaluator(args.gt_json, output_dir=args.output_dir, device=args.device)
    if args.gt_json:
        from .evaluation.ytvis import YTVISEvaluator
        return YTVISEvaluator(args.gt_json, output_dir=args.output_dir, device=args.device)
    if args.pan_gt_json:
        from .evaluation.vps import VPSEvaluator
        with open(args.pan_gt_json) as f:
            categories = {c["id"]: c for c in json.load(f)["categories"]}
        return VPSEvaluator(categories, args.pan_gt_json, args.truth_dir, args.output_dir, device=args.device,
                            png=getattr(args, "png", "host"), reader=getattr(args, "reader", "host"))
    # the two VOS evaluators read <their output_dir>/Annotations: the "inference" folder `write_vos_pngs` writes into
    if getattr(args, "davis_root", None):
        from .evaluation.davis import DAVISEvaluator      # (it takes the image root and drops two components: give them back)
        return DAVISEvaluator(args.dataset_name, os.path.join(args.davis_root, "JPEGImages", "Full-Resolution"),
                              output_dir=os.path.join(args.output_dir, "inference"), device=args.device,
                              reader=getattr(args, "reader", "host"))
    if getattr(args, "pvos_data", None):
        from .evaluation.pvos import PVOSEvaluator         # (likewise, one component)
        return PVOSEvaluator(args.dataset_name, os.path.join(args.pvos_data, "JPEGImages"), distributed=False,
                             output_dir=os.path.join(args.output_dir, "inference"), device=args.device,
                             reader=getattr(args, "reader", "host"))
    return None


def vos_clip_offsets(n_clips, num_frames, clip_stride):
    """The first frame of every clip's id maps.  `InferenceVideoVOS.inference_video_vos` starts clip c at frame c min(clip_stride,
    num_frames), and `_finished_frames` returns that clip's maps from its first frame on.  The running sum of the maps' lengths is the
    same number only while the stride is below the clip length: a clip that is not the last returns
    `mask_logits[:, -T : min(-T + stride, -1)]`, which is `stride` frames for stride < T but T - 1 frames for stride == T -- the clip's
    last frame is then in no clip's output (the reference's slice, inference_video_vos.py:640, kept as it is) and a running sum would
    drift by one frame per clip.  So the offsets come from the schedule, not from the lengths."""
    stride = min(int(clip_stride), int(num_frames))
    return [c * stride for c in range(n_clips)]


def write_vos_outputs(output_dir, inputs, outputs, num_frames, clip_stride, png="host"):
    """The per-clip id maps of one video ([T', H, W] uint8 each, `InferenceVideoVOS.save_vos_results`) -> the palette PNGs of
    `results.write_vos_pngs`, each clip at its offset (`vos_clip_offsets`).  Returns the paths."""
    video = inputs[0]
    paths = []
    for first, idmaps in zip(vos_clip_offsets(len(outputs), num_frames, clip_stride), outputs):
        paths += write_vos_pngs(output_dir, video["file_names"], first, idmaps, video.get("mask_palette"), png=png)
    return paths


def _legend(lut, names, present):
    """{row: {"name", "color", "alpha"}} of the rows that are drawn: those that occur in the id maps and are not transparent."""
    return {str(k): {"name": str(names.get(k, k)), "color": [int(c) for c in lut[k, :3]], "alpha": int(lut[k, 3])}
            for k in sorted(present) if lut[k, 3] > 0}


def _class_suffix(vocab, score):
    """": <name>" of the best class of a VIS result's per-class scores under an installed vocabulary; "" without one."""
    score = torch.as_tensor(score).reshape(-1)
    if vocab is None or score.numel() != len(vocab):
        return ""
    return ": " + vocab.names[int(score.argmax())]


def install_class_names(args, model):
    """--class-names: the vocabulary of the file, made by the model's own language encoder (or --clip-weights'), installed under
    --dataset-name, and O/inference/vocabulary.json (contiguous id -> name) beside the results."""
    from . import vocabulary
    tpe = getattr(model, "text_prompt_encoder", None)
    enc = getattr(tpe, "lang_encoder", None)
    if enc is None:
        if not args.clip_weights:
            raise SystemExit("--class-names: the config builds no language encoder; give --clip-weights")
        enc = vocabulary.build_lang_encoder(args.clip_weights, device=args.device)
    vocab = vocabulary.Vocabulary.from_file(args.class_names, enc)
    vocabulary.install(model, vocab, name=args.dataset_name, sub_task=args.sub_task or "vis")
    os.makedirs(os.path.join(args.output_dir, "inference"), exist_ok=True)
    with open(os.path.join(args.output_dir, "inference", "vocabulary.json"), "w") as f:
        json.dump({str(c): n for c, n in enumerate(vocab.names)}, f, indent=1)
    return vocab


def _category_table(args, alpha, n_default):
    """(lut, {row: name}, {category id: row}) from --categories-json ({"categories": [{"id", "name", "color"}]}), or without one the
    default palette with row = id + 1."""
    from .inference import overlay_rule as ov
    if getattr(args, "categories_json", None):
        with open(args.categories_json) as f:
            cats = {int(c["id"]): c for c in json.load(f)["categories"]}
        lut, order = ov.lut_from_categories(cats, alpha)
        return lut, {row: cats[cid].get("name", cid) for row, cid in enumerate(order) if cid is not None}, {cid: row for row, cid in enumerate(order)}
    lut = ov.lut_from_palette(ov.default_palette(n_default + 1), alpha)
    return lut, {}, None


def overlay_tables(args, inputs, outputs):
    """[(first frame, id maps [T', H, W], lut, {row: name})] of one video's output, or a sentence saying why it holds nothing to draw:
    the VOS driver's per-clip id maps with the video's palette; a VSS or VPS output's `pred_masks` with the category colours; VIS
    results that carry per-frame masks, through `idmap_from_instances`."""
    from .inference import overlay_rule as ov
    video = inputs[0]
    vocab = getattr(args, "vocabulary", None)                         # --class-names: row c + 1 is name c where no categories file names it
    vocab_names = {c + 1: n for c, n in enumerate(vocab.names)} if vocab is not None else {}
    if args.vos:
        vos = args.vos_schedule
        pal = video.get("mask_palette")
        lut = ov.lut_from_palette(pal if pal is not None else ov.default_palette())
        return [(first, m, lut, {}) for first, m in zip(vos_clip_offsets(len(outputs), *vos), outputs)]
    if isinstance(outputs, dict) and outputs.get("task") == "vss" and "pred_masks" in outputs:
        sem = torch.as_tensor(outputs["pred_masks"])
        lut, names, rows = _category_table(args, ov.ALPHA_VSS, int(sem.max()) + 1 if sem.numel() else 1)
        return [(0, sem + 1, lut, names or vocab_names)]              # contiguous class c: row c + 1 (row 0 is "nothing", transparent)
    if isinstance(outputs, dict) and outputs.get("task") == "vps" and "pred_masks" in outputs:
        pan = torch.as_tensor(outputs["pred_masks"]).long()
        infos = outputs["segments_infos"]
        lut, names, rows = _category_table(args, ov.ALPHA_VPS, max([int(i["category_id"]) for i in infos], default=0))
        ids = torch.zeros_like(pan, dtype=torch.int32)
        for info in infos:                                           # a segment is drawn in its category's colour
            row = rows.get(int(info["category_id"]), 0) if rows is not None else int(info["category_id"])
            ids[pan == int(info["id"])] = row
        return [(0, ids, lut, names or (vocab_names if rows is None else {}))]
    if isinstance(outputs, list) and outputs and all(isinstance(c, list) and all(isinstance(r, dict) and "masks" in r for r in c) for c in outputs):
        tables = []
        for clip in outputs:
            if not clip:
                continue
            masks = torch.stack([torch.as_tensor(r["masks"]) for r in clip])
            scores = torch.stack([torch.as_tensor(r["score"]).float().max() for r in clip])
            lut = ov.lut_from_palette(ov.default_palette(len(clip) + 1))
            tables.append((int(clip[0]["frame_id_start"]), ov.idmap_from_instances(masks, scores), lut,
                           {k + 1: "object %d" % r["obj_id"] + _class_suffix(vocab, r["score"]) for k, r in enumerate(clip)}))
        return tables
    return "the output holds no per-pixel result at the output size"


def write_overlays(args, inputs, outputs):
    """--visualize: the overlays of one video (`results.write_overlay_jpegs`) and its legend.json; the frames are read again at their
    original size, on the device with --decode gpu.  Returns the paths."""
    from .data import read_images
    from .inference.results import write_overlay_jpegs
    video = inputs[0]
    tables = overlay_tables(args, inputs, outputs)
    if isinstance(tables, str):
        print(f"--visualize: video {video.get('video_id')}: {tables}; nothing written")
        return []
    names = video["file_names"]
    frames = read_images(names, decode=args.decode, device=args.device if args.decode == "gpu" else None)
    paths, legend = [], {}
    for first, ids, lut, row_names in tables:
        n = min(len(ids), len(names) - first)
        paths += write_overlay_jpegs(args.output_dir, names, first, frames[first:first + n], ids[:n], lut, jpeg=args.visualize)
        present = torch.unique(torch.as_tensor(ids[:n]).long().clamp(0, len(lut) - 1)).tolist()
        legend.update(_legend(lut, row_names, present))
    if paths:
        with open(os.path.join(os.path.dirname(paths[0]), "legend.json"), "w") as f:
            json.dump(legend, f, indent=1, sort_keys=True)
    return paths


def main(argv=None):
    args = parse_args(argv)
    cfg = load_cfg(args.config_file, args.opts)
    model = build_model(cfg).eval()
    ckpt = torch.load(args.weights, map_location="cpu")
    model.load_state_dict(ckpt["model"], strict=True)
    model = model.to(args.device)
    if getattr(args, "class_names", None) is not None:
        args.vocabulary = install_class_names(args, model)
    if getattr(args, "image", False):
        run_images(args, cfg, model)
        return 0
    if args.vos and getattr(args, "masks_dir", None) is not None:
        records = vos_records_from_dirs(args.video_dir, args.masks_dir, args.dataset_name, meta_dir=args.vos_meta, reader=args.reader,
                                        device=args.device)
    elif args.vos:
        records = load_vos_json(args.json, args.image_root, args.dataset_name)
    elif args.json:
        records = load_video_json(args.json, args.image_root, args.dataset_name)
    else:
        records = video_records_from_dir(args.video_dir)
        if getattr(args, "vocabulary", None) is not None:           # the frames run as the installed vocabulary's data set
            for r in records:
                r["dataset_name"] = args.dataset_name
    mapper = (VOSTestMapper if args.vos else VideoTestMapper).from_config(cfg, resize=args.resize, device=args.device, decode=getattr(args, "decode", "host"))
    os.makedirs(args.output_dir, exist_ok=True)
    evaluator = build_evaluator(args)

    def save(inputs, outputs):
        torch.save(outputs, os.path.join(args.output_dir, f"{inputs[0]['video_id']}.pt"))

    def save_vos(inputs, outputs):
        vos = model.inference_video_vos
        write_vos_outputs(args.output_dir, inputs, outputs, vos.num_frames, vos.clip_stride, png=args.png)

    on_output = save_vos if args.vos else (None if evaluator is not None else save)
    if args.visualize != "off":
        if args.vos:
            args.vos_schedule = (model.inference_video_vos.num_frames, model.inference_video_vos.clip_stride)
        keep = on_output

        def on_output(inputs, outputs):
            if keep is not None:
                keep(inputs, outputs)
            write_overlays(args, inputs, outputs)
    results = inference_on_videos(model, records, mapper, evaluator, on_output=on_output)
    if evaluator is not None:
        print(json.dumps(results, default=str))
    return 0


if __name__ == "__main__":
    sys.exit(main())
