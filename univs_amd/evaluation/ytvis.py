"""AP / AR of a YouTube-VIS result (the records of `results.vis_clip_instances_to_coco_json_video`), from one overlap count per video
(vis_counts.py) instead of two `maskUtils.merge` and two `maskUtils.area` calls per (detection, ground truth, frame).

The reference scores with `YTVISEvaluator` (univs/evaluation/ytvis_evaluation.py:27-291) over `YTVOS.loadRes`
(univs/data/datasets/ytvis_api/ytvos.py:213-261) and `YTVOSeval` (ytvoseval.py:86-524).  Its IoU of two mask sequences, `iou_seq`
(ytvoseval.py:200-214), is I / (A_d + A_g - I): I the per-frame overlaps summed over the video, A the summed areas, 0.0 where the
denominator is 0; a `None` frame adds what an empty mask adds.  The sums are integers below 2^53, so the float64 quotient is the
reference's; everything after it (the greedy matching at ten thresholds, the precision / recall tables, the twelve summary numbers) is
host arithmetic on small tables, restated here with the reference's expressions and sort kinds so that the numbers come out the same.

  load_results     `YTVOS.loadRes`: ids from 1, `areas`, `avg_area` over the non-zero areas, `iscrowd = 0`, its two assertions
  YTVISEval        `YTVOSeval` for iouType 'segm' and the default parameters: evaluate / accumulate / summarize
  YTVISEvaluator   reset / process / evaluate / eval_predictions_by_files with the reference's call pattern, without its tables and logs

Per video there is ONE overlap call, all of its detections against all of its ground truths; the blocks ious[(video, category)] are
cut from that table, rows in the reference's order (stable sort by -score, cut at maxDets[-1]).  Records that share one
`segmentations` list -- the (entity, class) records of one entity -- are counted once.

Not restated: polygon segmentations (NotImplementedError: pycocotools' rasteriser is absent here and cannot be pinned), the 'bbox' and
'keypoints' types, `bboxes` of the loaded results (the 'segm' scores never read them).  Stricter than the reference: a mask whose size is
not its video's, and mask sequences of different lengths inside one video (the reference's `zip` would drop the tail silently), are a
ValueError that names the video.

`python -m univs_amd.evaluation.ytvis --gt_json ... --results ...` prints the twelve summary lines.  Single process.
"""
import argparse
import copy
import json
import os
import sys
from collections import OrderedDict, defaultdict

import numpy as np
import torch

from ._counts import pick_device as _device
from .vis_counts import runs_from_rles, vis_overlap

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 128 ** 2), (128 ** 2, 256 ** 2), (256 ** 2, 1e5 ** 2))
AREA_LBL = ("all", "small", "medium", "large")
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")


def _avg_area(areas):
    kept = [a for a in areas if a]
    return 0 if len(kept) == 0 else np.array(kept).mean()


def _video_runs(anns, video, device=None):
    """The masks of `anns` (records of ONE video) as Runs, object-major; a `segmentations` list that several records share is taken
    once -> (runs, row of every record, T)."""
    rows, lists, seen = [], [], {}
    for a in anns:
        key = id(a["segmentations"])
        if key not in seen:
            seen[key] = len(lists)
            lists.append(a["segmentations"])
        rows.append(seen[key])
    T = len(lists[0])
    if any(len(s) != T for s in lists):
        raise ValueError(f"video {video['id']}: mask sequences of {sorted(set(len(s) for s in lists))} frames")
    runs = runs_from_rles([m for s in lists for m in s], video["height"], video["width"], device=device, video=video["id"])
    return runs, np.asarray(rows, dtype=np.int64), T


def load_results(dataset, anns):
    """`YTVOS.loadRes` on the annotation dictionary `dataset` and the result list `anns` -> (records, per video: (runs, rows, T)).
    The records are shallow copies (a shared `segmentations` list stays shared) with `id` (from 1, in order), `areas` (one per frame,
    None where there is no mask), `avg_area` (the mean of the non-zero areas, 0 without any) and `iscrowd` = 0."""
    assert type(anns) == list, 'results in not an array of objects'
    videos = {v["id"]: v for v in dataset["videos"]}
    assert set(a["video_id"] for a in anns) <= set(videos), 'Results do not correspond to current coco set'
    if "segmentations" not in anns[0]:
        raise ValueError("the results hold no 'segmentations': only mask results are scored")
    anns = [dict(a) for a in anns]
    by_video = defaultdict(list)
    for i, a in enumerate(anns):
        a["id"] = i + 1
        a["iscrowd"] = 0
        by_video[a["video_id"]].append(a)
    per_video = {}
    for vid, recs in by_video.items():
        runs, rows, T = _video_runs(recs, videos[vid])
        area = runs.areas().reshape(-1, T).numpy()
        for a, r in zip(recs, rows):
            a["areas"] = [int(area[r, t]) if m else None for t, m in enumerate(a["segmentations"])]
            a["avg_area"] = _avg_area(a["areas"])
        per_video[vid] = (runs, rows, T)
    return anns, per_video


class YTVISEval:
    """`YTVOSeval(cocoGt, cocoDt, 'segm')` with the default `Params`: iouThrs .5:.05:.95, recThrs 0:.01:1, maxDets 1 / 10 / 100, the four
    area ranges on `avg_area`, categories used.  After evaluate / accumulate / summarize: `ious` {(video, category): float64 [D, G], or
    [] where there is neither}, `eval` {'precision' [T, R, K, A, M], 'recall' [T, K, A, M], 'scores'}, `stats` [12], `summary` (the
    twelve lines the reference prints)."""

    area_rng = AREA_RNG                      # (evaluation/coco.py: COCOSegmEval shares everything below _video_ious and has COCO's ranges)

    def __init__(self, dataset, results, device=None):
        self.dataset, self.device = dataset, _device(device)
        self.videos = {v["id"]: v for v in dataset["videos"]}
        self.vid_ids = list(np.unique(sorted(self.videos)))
        self.cat_ids = list(np.unique(sorted(c["id"] for c in dataset["categories"])))
        self.dts, self.dt_runs = load_results(dataset, results)
        self.ious, self.eval, self.stats, self.summary = {}, {}, [], []

    # ---- _prepare + computeIoU ------------------------------------------------------------------------------------------------------
    def _prepare(self):
        cats = set(self.cat_ids)
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        self._gt_col, self._dt_row = {}, {}
        gt_by_video = defaultdict(list)
        for g in self.dataset["annotations"]:
            gt_by_video[g["video_id"]].append(g)
        self._gt_by_video = gt_by_video
        for vid in self.vid_ids:
            for g in gt_by_video.get(vid, ()):
                g["avg_area"] = _avg_area(g["areas"])
                g["ignore"] = 'iscrowd' in g and g['iscrowd']
                if g["category_id"] in cats:
                    self._gts[vid, g["category_id"]].append(g)
        dt_by_video = defaultdict(list)
        for d in self.dts:
            dt_by_video[d["video_id"]].append(d)
        for vid in self.vid_ids:
            for d, r in zip(dt_by_video.get(vid, ()), self.dt_runs[vid][1] if vid in self.dt_runs else ()):
                self._dt_row[id(d)] = int(r)
                if d["category_id"] in cats:
                    self._dts[vid, d["category_id"]].append(d)

    def _video_ious(self, vid):
        """float64 [unique detection sequences, ground truths] of one video, or None where a side is empty."""
        gts = self._gt_by_video.get(vid, ())
        if vid not in self.dt_runs or len(gts) == 0:
            return None
        video = self.videos[vid]
        dt_runs, _, T = self.dt_runs[vid]
        gt_runs, gt_rows, Tg = _video_runs(gts, video)
        if Tg != T:
            raise ValueError(f"video {vid}: results of {T} frames, annotations of {Tg}")
        for g, r in zip(gts, gt_rows):
            self._gt_col[id(g)] = int(r)
        inter = vis_overlap(dt_runs.to(self.device), gt_runs.to(self.device), T, video["height"], video["width"])
        i = inter.to(torch.int64).sum(dim=2).cpu().numpy()
        a_d = dt_runs.areas().reshape(-1, T).sum(dim=1).numpy()
        a_g = gt_runs.areas().reshape(-1, T).sum(dim=1).numpy()
        u = a_d[:, None] + a_g[None, :] - i
        return np.where(u > 0, i.astype(np.float64) / np.where(u > 0, u, 1).astype(np.float64), 0.0)

    def evaluate(self):
        self._prepare()
        top = MAX_DETS[-1]
        self.ious = {}
        for vid in self.vid_ids:
            table = self._video_ious(vid)
            for cat in self.cat_ids:
                gt, dt = self._gts[vid, cat], self._dts[vid, cat]
                if len(gt) == 0 and len(dt) == 0:
                    self.ious[vid, cat] = []
                    continue
                order = np.argsort([-d["score"] for d in dt], kind="mergesort")[:top]
                if table is None:
                    self.ious[vid, cat] = np.zeros([len(order), len(gt)])
                else:
                    rows = [self._dt_row[id(dt[i])] for i in order]
                    cols = [self._gt_col[id(g)] for g in gt]
                    self.ious[vid, cat] = table[np.ix_(rows, cols)].reshape(len(rows), len(cols))
        self.eval_vids = [self._evaluate_vid(vid, cat, rng, top) for cat in self.cat_ids for rng in self.area_rng for vid in self.vid_ids]

    # ---- evaluateVid ---------------------------------------------------------------------------------------------------------------------
    def _evaluate_vid(self, vid, cat, rng, max_det):
        gt, dt = self._gts[vid, cat], self._dts[vid, cat]
        if len(gt) == 0 and len(dt) == 0:
            return None
        for g in gt:
            g["_ignore"] = 1 if g["ignore"] or (g["avg_area"] < rng[0] or g["avg_area"] > rng[1]) else 0
        gt_order = np.argsort([g["_ignore"] for g in gt], kind="mergesort")      # ignored ground truths last
        gt = [gt[i] for i in gt_order]
        dt_order = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dt_order[0:max_det]]
        crowd = [int(g["iscrowd"]) for g in gt]
        ious = self.ious[vid, cat]
        if len(ious) > 0:
            ious = ious[:, gt_order]
        n_thr, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm, dtm = np.zeros((n_thr, G)), np.zeros((n_thr, D))
        gt_ig = np.array([g["_ignore"] for g in gt])
        dt_ig = np.zeros((n_thr, D))
        if len(ious) != 0:
            for ti, thr in enumerate(IOU_THRS):
                for di, d in enumerate(dt):
                    best, m = min([thr, 1 - 1e-10]), -1
                    for gi in range(G):
                        if gtm[ti, gi] > 0 and not crowd[gi]:                   # taken, and no crowd
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gi] == 1:         # matched to a counted one: the ignored ones follow
                            break
                        if ious[di, gi] < best:
                            continue
                        best, m = ious[di, gi], gi
                    if m == -1:
                        continue
                    dt_ig[ti, di] = gt_ig[m]
                    dtm[ti, di] = gt[m]["id"]
                    gtm[ti, m] = d["id"]
        outside = np.array([d["avg_area"] < rng[0] or d["avg_area"] > rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(outside, n_thr, 0)))
        return {"dtMatches": dtm, "gtMatches": gtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig,
                "dtIds": [d["id"] for d in dt], "gtIds": [g["id"] for g in gt]}

    # ---- accumulate ----------------------------------------------------------------------------------------------------------------------
    def accumulate(self):
        n_thr, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(self.area_rng), len(MAX_DETS)
        I = len(self.vid_ids)
        precision = -np.ones((n_thr, R, K, A, M))
        recall = -np.ones((n_thr, K, A, M))
        scores = -np.ones((n_thr, R, K, A, M))
        for k in range(K):
            for a in range(A):
                E = [e for e in self.eval_vids[(k * A + a) * I:(k * A + a + 1) * I] if e is not None]
                if len(E) == 0:
                    continue
                for m, max_det in enumerate(MAX_DETS):
                    dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                    order = np.argsort(-dt_scores, kind="mergesort")
                    sorted_scores = dt_scores[order]
                    dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, order]
                    dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, order]
                    gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gt_ig == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t in range(n_thr):
                        tp, fp = tp_sum[t], fp_sum[t]
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = np.maximum.accumulate(pr[::-1])[::-1]               # the envelope: pr[i - 1] = max(pr[i - 1], pr[i]) from the end
                        at = np.searchsorted(rc, REC_THRS, side="left")
                        ok = at < nd                                             # a prefix (at is sorted): the reference's loop stops at the first miss
                        q, ss = np.zeros((R,)), np.zeros((R,))
                        q[ok], ss[ok] = pr[at[ok]], sorted_scores[at[ok]]
                        precision[t, :, k, a, m] = q
                        scores[t, :, k, a, m] = ss
        self.eval = {"counts": [n_thr, R, K, A, M], "precision": precision, "recall": recall, "scores": scores}

    # ---- summarize -----------------------------------------------------------------------------------------------------------------------
    def _summarize(self, ap=1, iou_thr=None, area="all", max_dets=100):
        line = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'
        title, kind = ('Average Precision', '(AP)') if ap == 1 else ('Average Recall', '(AR)')
        iou = '{:0.2f}:{:0.2f}'.format(IOU_THRS[0], IOU_THRS[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr)
        aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
        mind = [i for i, md in enumerate(MAX_DETS) if md == max_dets]
        s = self.eval["precision"] if ap == 1 else self.eval["recall"]
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        mean = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        self.summary.append(line.format(title, kind, iou, area, max_dets, mean))
        return mean

    def summarize(self):
        if not self.eval:
            raise Exception('Please run accumulate() first')
        self.summary = []
        top = MAX_DETS[2]
        stats = np.zeros((12,))
        stats[0] = self._summarize(1)
        stats[1] = self._summarize(1, iou_thr=.5, max_dets=top)
        stats[2] = self._summarize(1, iou_thr=.75, max_dets=top)
        for i, lbl in enumerate(AREA_LBL[1:]):
            stats[3 + i] = self._summarize(1, area=lbl, max_dets=top)
        for i, md in enumerate(MAX_DETS):
            stats[6 + i] = self._summarize(0, max_dets=md)
        for i, lbl in enumerate(AREA_LBL[1:]):
            stats[9 + i] = self._summarize(0, area=lbl, max_dets=top)
        self.stats = stats


def evaluate_predictions_on_ytvis(dataset, results, device=None):
    """`_evaluate_predictions_on_ytvis`: load, evaluate, accumulate, summarize -> YTVISEval."""
    e = YTVISEval(dataset, results, device=device)
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e


def derive_coco_results(vis_eval, class_names=None):
    """`YTVISEvaluator._derive_coco_results` for 'segm': AP, AP50, AP75, APs, APm, APl in percent (NaN for a negative summary), and
    with more than one class name 'AP-<name>' per category: the mean of its precisions above -1 over all areas at maxDets[-1]."""
    if vis_eval is None:
        return {m: float("nan") for m in METRICS}
    results = {m: float(vis_eval.stats[i] * 100 if vis_eval.stats[i] >= 0 else "nan") for i, m in enumerate(METRICS)}
    if class_names is None or len(class_names) <= 1:
        return results
    precisions = vis_eval.eval["precision"]
    assert len(class_names) == precisions.shape[2]
    for k, name in enumerate(class_names):
        p = precisions[:, :, k, 0, -1]
        p = p[p > -1]
        results["AP-" + "{}".format(name)] = float((np.mean(p) if p.size else float("nan")) * 100)
    return results


def instances_to_coco_json_video(inputs, outputs):
    """The records of one video from {"pred_scores", "pred_labels", "pred_masks" (per instance [T, H, W])}; all masks are encoded in one
    `rle_encode_masks` call."""
    from ..inference.results import rle_encode_masks
    assert len(inputs) == 1, "More than one inputs are loaded for inference!"
    video_id, height, width = int(inputs[0]["video_id"]), int(inputs[0]["height"]), int(inputs[0]["width"])
    scores, labels, masks = outputs["pred_scores"], outputs["pred_labels"], outputs["pred_masks"]
    masks = [torch.as_tensor(m) for m in masks]
    rles = rle_encode_masks(torch.cat([m.reshape(-1, *m.shape[-2:]) for m in masks], dim=0)) if len(masks) else []
    out, o = [], 0
    for s, l, m in zip(scores, labels, masks):
        out.append({"video_id": video_id, "score": s, "category_id": l, "segmentations": rles[o:o + m.shape[0]], "height": height,
                    "width": width})
        o += m.shape[0]
    return out


class YTVISEvaluator:
    """`YTVISEvaluator` without detectron2's catalog: the annotation file (a path or the loaded dictionary), optionally the class names
    (per-category AP), the category-id mapping of the data set (`thing_dataset_id_to_contiguous_id`: predictions are unmapped before
    they are written and scored), the output directory (`instances_predictions.pth`, `results.json`) and the device of the counts."""

    def __init__(self, gt_json, thing_classes=None, output_dir=None, device=None, thing_dataset_id_to_contiguous_id=None):
        if isinstance(gt_json, (str, os.PathLike)):
            with open(gt_json, "r") as f:
                gt_json = json.load(f)
        assert type(gt_json) == dict, 'annotation file format {} not supported'.format(type(gt_json))
        self._dataset = gt_json
        if "annotations" in self._dataset and self._dataset["annotations"] is None:
            self._dataset.pop("annotations")
        self._do_evaluation = "annotations" in self._dataset
        self._thing_classes, self._output_dir, self._device = thing_classes, output_dir, device
        self._id_map = thing_dataset_id_to_contiguous_id
        self.last_eval = None
        self.reset()

    def reset(self):
        self._predictions = []

    def process(self, inputs, outputs):
        if isinstance(outputs, dict):
            prediction = instances_to_coco_json_video(inputs, outputs)
        elif isinstance(outputs, list):
            prediction = outputs
        else:
            raise ValueError
        self._predictions.extend(prediction)

    def evaluate(self):
        predictions = self._predictions
        if len(predictions) == 0:
            return {}
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, "instances_predictions.pth"), "wb") as f:
                torch.save(predictions, f)
        self._results = OrderedDict()
        self._eval_predictions(predictions)
        return copy.deepcopy(self._results)

    def _eval_predictions(self, predictions):
        if self._id_map is not None:
            contiguous = list(self._id_map.values())
            num_classes = len(contiguous)
            assert min(contiguous) == 0 and max(contiguous) == num_classes - 1
            reverse = {v: k for k, v in self._id_map.items()}
            if num_classes > 1:
                for result in predictions:
                    category_id = result["category_id"]
                    assert category_id < num_classes, (f"A prediction has class={category_id}, but the dataset only has {num_classes} classes "
                                                       f"and predicted class id should be in [0, {num_classes - 1}].")
                    result["category_id"] = reverse[category_id]
        if self._output_dir:
            with open(os.path.join(self._output_dir, "results.json"), "w") as f:
                f.write(json.dumps(predictions))
                f.flush()
        if not self._do_evaluation:
            return
        self.last_eval = evaluate_predictions_on_ytvis(self._dataset, predictions, device=self._device)
        self._results["segm"] = derive_coco_results(self.last_eval, class_names=self._thing_classes)

    def eval_predictions_by_files(self, pred_results_file):
        with open(pred_results_file, "r") as f:
            predictions = json.load(f)
        self.last_eval = evaluate_predictions_on_ytvis(self._dataset, predictions, device=self._device)
        return derive_coco_results(self.last_eval, class_names=self._thing_classes)


def main(argv=None):
    ap = argparse.ArgumentParser(description="AP / AR of a YouTube-VIS result file")
    ap.add_argument("--gt_json", required=True, help="the annotation file (YouTube-VIS format, with `annotations`)")
    ap.add_argument("--results", required=True, help="results.json: the list of result records")
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    ev = YTVISEvaluator(args.gt_json, device=args.device)
    ev.eval_predictions_by_files(args.results)
    for line in ev.last_eval.summary:
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
