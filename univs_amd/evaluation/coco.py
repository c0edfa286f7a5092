"""COCO instance mask AP / AR of a per-image result (the records of `results.image_instances_to_coco_json`), from one polygon
rasterisation of the whole annotation file (polygon_ops.py, csrc/polygon_runs.hip) and one overlap count per image (vis_counts.py).

`COCOSegmEval` is COCOeval with iouType 'segm' and the default parameters.  The reference's YouTube-VIS scorer (`ytvoseval.py`) is a
copy of COCOeval, and `ytvis.YTVISEval` restates it and is pinned to it; an image is a video of one frame, so everything after the IoU
table -- the greedy matching at ten thresholds, accumulate, summarize -- is YTVISEval's own code, inherited.  What differs:

  * images instead of videos (T = 1), `image_id` and `segmentation` instead of `video_id` and `segmentations`;
  * the area ranges [0, 1e10], [0, 32^2], [32^2, 96^2], [96^2, 1e10];
  * a ground truth's area is the json's `area`, a detection's area is its mask's;
  * the IoU against a crowd ground truth is I / A_d;
  * a union of 0 is IoU 0, as in YTVISEval: this project's choice (pycocotools' own answer is not available to compare with).

The ground truth's segmentations -- polygons, and the uncompressed RLE of crowd regions -- are rasterised in ONE
`runs_from_segmentations` call and stay on the device; per image `vis_overlap(dt, gt, 1, H, W)` gives the intersections.  The polygon
rule is data/polygon_rule.py, this project's restatement of the COCO API's published one: pinned by hand-derivable cases and anchors,
not by pycocotools' code, which is not available here.  A mask whose size is not its image's is a ValueError that names the image.

`python -m univs_amd.evaluation.coco --gt_json G --results R` prints the twelve summary lines.  Single process.
"""
import argparse
import copy
import json
import os
import sys
from collections import OrderedDict, defaultdict

import numpy as np

from ..polygon_ops import runs_from_segmentations, slice_runs
from .vis_counts import vis_overlap
from .ytvis import YTVISEval, derive_coco_results

AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))


def _by_image(anns, vid_ids):
    """`anns` in the order of `vid_ids`, file order inside an image (COCO.getAnnIds) -> (sorted list, {image: (first, end)})."""
    per = defaultdict(list)
    for a in anns:
        per[a["image_id"]].append(a)
    out, rng = [], {}
    for vid in vid_ids:
        rng[vid] = (len(out), len(out) + len(per.get(vid, ())))
        out.extend(per.get(vid, ()))
    return out, rng


class COCOSegmEval(YTVISEval):
    """`COCOeval(cocoGt, cocoDt, 'segm')` with the default `Params`.  `gt_dataset`: the loaded instances json (images, annotations,
    categories); `results`: the list of result records.  After evaluate / accumulate / summarize: `ious`, `eval`, `stats` [12],
    `summary`, as in YTVISEval."""

    area_rng = AREA_RNG

    def __init__(self, gt_dataset, results, device=None):
        from ._counts import pick_device
        self.dataset, self.device = gt_dataset, pick_device(device)
        self.videos = {im["id"]: im for im in gt_dataset["images"]}
        self.vid_ids = list(np.unique(sorted(self.videos)))
        self.cat_ids = list(np.unique(sorted(c["id"] for c in gt_dataset["categories"])))
        assert type(results) == list, 'results in not an array of objects'
        assert set(r["image_id"] for r in results) <= set(self.videos), 'Results do not correspond to current coco set'
        if results and "segmentation" not in results[0]:
            raise ValueError("the results hold no 'segmentation': only mask results are scored")
        self.dts = [dict(r) for r in results]
        for i, d in enumerate(self.dts):                                  # COCO.loadRes
            d["id"], d["iscrowd"] = i + 1, 0
        self._dt_sorted, self._dt_range = _by_image(self.dts, self.vid_ids)
        self._gt_sorted, self._gt_range = _by_image([dict(g) for g in gt_dataset.get("annotations", ())], self.vid_ids)
        self.gt_runs = self._rasterise(self._gt_sorted, "annotation")     # ONE call for the file; stays on the device
        self.dt_runs = self._rasterise(self._dt_sorted, "result")
        self._gt_starts, self._dt_starts = self.gt_runs.starts.cpu().numpy(), self.dt_runs.starts.cpu().numpy()
        self._gt_area, self._dt_area = self.gt_runs.areas().cpu().numpy(), self.dt_runs.areas().cpu().numpy()
        for d, a in zip(self._dt_sorted, self._dt_area):
            d["area"] = d["avg_area"] = int(a)
        self.ious, self.eval, self.stats, self.summary = {}, {}, [], []

    def _rasterise(self, anns, kind):
        sizes = [(self.videos[a["image_id"]]["height"], self.videos[a["image_id"]]["width"]) for a in anns]
        names = [f"image {a['image_id']}, {kind} {a.get('id')}" for a in anns]
        return runs_from_segmentations([a.get("segmentation") for a in anns], sizes, self.device, names)

    def _prepare(self):
        cats = set(self.cat_ids)
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        self._gt_col, self._dt_row = {}, {}
        for vid in self.vid_ids:
            a, b = self._gt_range[vid]
            for col, g in enumerate(self._gt_sorted[a:b]):
                g.setdefault("iscrowd", 0)
                g["avg_area"] = g["area"]
                g["ignore"] = g["iscrowd"]
                self._gt_col[id(g)] = col
                if g["category_id"] in cats:
                    self._gts[vid, g["category_id"]].append(g)
            a, b = self._dt_range[vid]
            for row, d in enumerate(self._dt_sorted[a:b]):
                self._dt_row[id(d)] = row
                if d["category_id"] in cats:
                    self._dts[vid, d["category_id"]].append(d)

    def _video_ious(self, vid):
        """float64 [detections, ground truths] of one image, or None where a side is empty."""
        (g0, g1), (d0, d1) = self._gt_range[vid], self._dt_range[vid]
        if g0 == g1 or d0 == d1:
            return None
        im = self.videos[vid]
        dt, gt = slice_runs(self.dt_runs, d0, d1, self._dt_starts), slice_runs(self.gt_runs, g0, g1, self._gt_starts)
        i = vis_overlap(dt, gt, 1, im["height"], im["width"])[:, :, 0].cpu().numpy().astype(np.int64)
        a_d, a_g = self._dt_area[d0:d1], self._gt_area[g0:g1]
        crowd = np.array([bool(g.get("iscrowd", 0)) for g in self._gt_sorted[g0:g1]])
        u = np.where(crowd[None, :], np.broadcast_to(a_d[:, None], i.shape), a_d[:, None] + a_g[None, :] - i)
        return np.where(u > 0, i.astype(np.float64) / np.where(u > 0, u, 1).astype(np.float64), 0.0)


def evaluate_predictions_on_coco(gt_dataset, results, device=None):
    e = COCOSegmEval(gt_dataset, results, device=device)
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e


class COCOInstanceEvaluator:
    """reset / process / evaluate around `COCOSegmEval`.  `gt_json`: an instances json (a path or the loaded dictionary).  `process`
    takes the records of `image_instances_to_coco_json`; an `image_id` that is no id of the file is looked up as the stem of an image's
    `file_name` (an --image-dir run names its images by their files).  `evaluate` -> {"segm": {AP, AP50, AP75, APs, APm, APl, AP-<name>
    ...}} and, with an output directory, `coco-segm-ap.txt`: the twelve summary lines."""

    def __init__(self, gt_json, output_dir=None, device=None):
        if isinstance(gt_json, (str, os.PathLike)):
            with open(gt_json, "r") as f:
                gt_json = json.load(f)
        assert type(gt_json) == dict, 'annotation file format {} not supported'.format(type(gt_json))
        self._dataset, self._output_dir, self._device = gt_json, output_dir, device
        self._ids = {im["id"]: im["id"] for im in gt_json["images"]}
        self._stems = {os.path.splitext(os.path.basename(im["file_name"]))[0]: im["id"] for im in gt_json["images"] if "file_name" in im}
        cats = sorted(gt_json["categories"], key=lambda c: c["id"])
        self._class_names = [c.get("name", str(c["id"])) for c in cats]
        self.last_eval = None
        self.reset()

    def reset(self):
        self._predictions = []

    def _image_id(self, key):
        if key in self._ids:
            return key
        if key in self._stems:
            return self._stems[key]
        raise ValueError(f"image {key!r} of the results is neither an image id nor a file name of the ground truth")

    def process(self, records):
        self._predictions.extend(records)

    def evaluate(self):
        results = []
        for r in self._predictions:
            r = dict(r)
            r["image_id"] = self._image_id(r["image_id"])
            results.append(r)
        self.last_eval = evaluate_predictions_on_coco(self._dataset, results, device=self._device)
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, "coco-segm-ap.txt"), "w") as f:
                f.write("\n".join(self.last_eval.summary) + "\n")
        out = OrderedDict()
        out["segm"] = derive_coco_results(self.last_eval, class_names=self._class_names)
        return copy.deepcopy(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description="mask AP / AR of a COCO instance result file")
    ap.add_argument("--gt_json", required=True, help="the annotation file (COCO instances format: polygons, RLE for crowd regions)")
    ap.add_argument("--results", required=True, help="coco_instances_results.json: the list of result records")
    ap.add_argument("--output_dir", default=None, help="where coco-segm-ap.txt is written")
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    ev = COCOInstanceEvaluator(args.gt_json, output_dir=args.output_dir, device=args.device)
    with open(args.results, "r") as f:
        ev.process(json.load(f))
    ev.evaluate()
    for line in ev.last_eval.summary:
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
