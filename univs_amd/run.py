"""`python -m univs_amd.run`: a checkpoint and frames on disk to result files.

    python -m univs_amd.run --config-file F --weights W (--json J --image-root R --dataset-name N | --video-dir D) --output-dir O
                            [--resize gpu|host] [--gt-json G | --pan-gt-json P --truth-dir T] [KEY VALUE ...]

The model is `build_model(load_cfg(F, [KEY VALUE ...]))` with `ckpt["model"]` loaded strictly (the reference's state-dict layout).  The
frames are the videos of a YouTube-VIS-format file, or the sub-folders of a folder of jpg / png frames (data/datasets.py), mapped by
data.VideoTestMapper.  With --gt-json the outputs go to evaluation.YTVISEvaluator (results.json; AP / AR when the file has annotations),
with --pan-gt-json and --truth-dir to evaluation.VPSEvaluator; without either each video's driver output is saved to O/<video_id>.pt.
"""
import argparse
import json
import os
import sys

import torch

from .config import load_cfg
from .data import VideoTestMapper, load_video_json, video_records_from_dir
from .engine import inference_on_videos
from .modeling.build import build_model


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m univs_amd.run", description="video inference from files on disk")
    ap.add_argument("--config-file", required=True)
    ap.add_argument("--weights", required=True, help="a checkpoint whose \"model\" entry is the state dict")
    ap.add_argument("--json", help="a YouTube-VIS-format test file")
    ap.add_argument("--image-root", help="the folder the file names of --json are relative to")
    ap.add_argument("--dataset-name", help="the registered name of --json's data set, e.g. ytvis_2021_val")
    ap.add_argument("--video-dir", help="a folder whose sub-folders hold the frames of one video each")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--resize", choices=("gpu", "host"), default="gpu")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--gt-json", help="YouTube-VIS annotation file: score with YTVISEvaluator")
    ap.add_argument("--pan-gt-json", help="VIPSeg panoptic ground-truth json: score with VPSEvaluator (with --truth-dir)")
    ap.add_argument("--truth-dir", help="the folder of the ground-truth panoptic PNGs")
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE pairs merged into the config")
    args = ap.parse_args(argv)
    from_json = args.json is not None
    if from_json == (args.video_dir is not None):
        ap.error("give either --json (with --image-root and --dataset-name) or --video-dir")
    if from_json and not (args.image_root and args.dataset_name):
        ap.error("--json needs --image-root and --dataset-name")
    if (args.pan_gt_json is None) != (args.truth_dir is None):
        ap.error("--pan-gt-json and --truth-dir go together")
    if args.gt_json and args.pan_gt_json:
        ap.error("one evaluator at a time: --gt-json or --pan-gt-json")
    return args


def build_evaluator(args):
    if args.gt_json:
        from .evaluation.ytvis import YTVISEvaluator
        return YTVISEvaluator(args.gt_json, output_dir=args.output_dir, device=args.device)
    if args.pan_gt_json:
        from .evaluation.vps import VPSEvaluator
        with open(args.pan_gt_json) as f:
            categories = {c["id"]: c for c in json.load(f)["categories"]}
        return VPSEvaluator(categories, args.pan_gt_json, args.truth_dir, args.output_dir, device=args.device)
    return None


def main(argv=None):
    args = parse_args(argv)
    cfg = load_cfg(args.config_file, args.opts)
    model = build_model(cfg).eval()
    ckpt = torch.load(args.weights, map_location="cpu")
    model.load_state_dict(ckpt["model"], strict=True)
    model = model.to(args.device)
    if args.json:
        records = load_video_json(args.json, args.image_root, args.dataset_name)
    else:
        records = video_records_from_dir(args.video_dir)
    mapper = VideoTestMapper.from_config(cfg, resize=args.resize, device=args.device)
    os.makedirs(args.output_dir, exist_ok=True)
    evaluator = build_evaluator(args)

    def save(inputs, outputs):
        torch.save(outputs, os.path.join(args.output_dir, f"{inputs[0]['video_id']}.pt"))

    results = inference_on_videos(model, records, mapper, evaluator, on_output=None if evaluator is not None else save)
    if evaluator is not None:
        print(json.dumps(results, default=str))
    return 0


if __name__ == "__main__":
    sys.exit(main())
