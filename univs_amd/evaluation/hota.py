"""HOTA of a tracking result (the records of `results.vis_clip_instances_to_coco_json_video`, or id maps), from one overlap count and
one launch of the HOTA tables per video (vis_counts.py, hota_counts.py) instead of three Python frame loops with a scipy assignment per
frame.

The metric is the reference's `HOTA` (univs/evaluation/eval_hota.py, TrackEval's class over univs/evaluation/_base_metric.py):
`eval_sequence`, `combine_sequences`, `combine_classes_class_averaged`, `combine_classes_det_averaged`, `_compute_final_fields`, restated
here with its field names, its `array_labels = np.arange(0.05, 0.99, 0.05)` and its `alpha - np.finfo('float').eps` comparison.  The
frame loops of `eval_sequence` are the tables of hota_counts.py; what follows them (AssA / AssRe / AssPr, LocA, the final fields, the
combinations) is host arithmetic on small arrays with the reference's numpy expressions, so that the numbers come out the same.

The protocol.  The reference holds no TrackEval dataset class, so the data protocol around the metric is this project's own:
  * inputs are a YouTube-VIS-format ground-truth file and result records (the `YTVISEvaluator` inputs); masks are read with
    `runs_from_rles` (polygons stay its NotImplementedError);
  * one sequence is one (video, category): the ground-truth tracks of that category and the result tracks predicted as it; result tracks
    with `score < score_thresh` are dropped (`score_thresh` defaults to 0); `iscrowd` ground-truth tracks are dropped;
  * with `class_agnostic=True` a video is one sequence of the single class "all" (the BURST / VOS use);
  * an id is present in frame t iff its mask there is not None and has area > 0;
  * similarity[g, p] = I / (A_g + A_p - I) in float64;
  * `num_gt_ids` / `num_tracker_ids` are the tracks of the sequence, `num_gt_dets` / `num_tracker_dets` the sums of their presences;
  * a (video, category) with neither ground truth nor results is no sequence, and a category without any sequence is left out of the
    per-class results and of both class combinations (it would add nothing to a sum and a 0 / LocA = 1 row to the class average).
Stricter than a silent `zip`: mask sequences of different lengths inside a video, a mask whose size is not its video's (ValueError that
names the video), a result for a video the ground truth does not list (AssertionError, `YTVOS.loadRes`'s sentence).

Not restated: TrackEval's dataset preprocessing (BURST's LVIS class split, ignore regions), polygons, the matplotlib plot.

  HOTAEvaluator        reset / process / evaluate, the pattern of `YTVISEvaluator`; every video is counted during `process`
  evaluate_hota_files  a ground-truth file and a result file -> the result dictionary
  hota_from_idmaps     id maps [T, H, W] of both sides (0 = background) -> the result of the one class-agnostic sequence, over `pair_counts`

`python -m univs_amd.evaluation.hota --gt_json ... --results ... [--score_thresh S] [--class_agnostic]` prints the summary and
writes it to hota-final.txt beside the result file (or into --output_dir).  Single process.
"""
import argparse
import json
import os
import sys
from collections import OrderedDict, defaultdict

import numpy as np
import torch

from ._counts import pick_device as _device
from .hota_counts import EPS, hota_counts
from .pair_counts import pair_counts
from .vis_counts import vis_overlap
from .ytvis import _video_runs, instances_to_coco_json_video

ARRAY_LABELS = np.arange(0.05, 0.99, 0.05)
THRESHOLDS = np.array([alpha - EPS for alpha in ARRAY_LABELS])
INTEGER_ARRAY_FIELDS = ['HOTA_TP', 'HOTA_FN', 'HOTA_FP']
FLOAT_ARRAY_FIELDS = ['HOTA', 'DetA', 'AssA', 'DetRe', 'DetPr', 'AssRe', 'AssPr', 'LocA', 'OWTA']
FLOAT_FIELDS = ['HOTA(0)', 'LocA(0)', 'HOTALocA(0)']
FIELDS = FLOAT_ARRAY_FIELDS + INTEGER_ARRAY_FIELDS + FLOAT_FIELDS
SUMMARY_FIELDS = FLOAT_ARRAY_FIELDS + FLOAT_FIELDS
ALL = "all"            # the one class of a class-agnostic evaluation


# ---- the metric (eval_hota.py) ---------------------------------------------------------------------------------------------------------------
def _compute_final_fields(res):
    res['DetRe'] = res['HOTA_TP'] / np.maximum(1, res['HOTA_TP'] + res['HOTA_FN'])
    res['DetPr'] = res['HOTA_TP'] / np.maximum(1, res['HOTA_TP'] + res['HOTA_FP'])
    res['DetA'] = res['HOTA_TP'] / np.maximum(1, res['HOTA_TP'] + res['HOTA_FN'] + res['HOTA_FP'])
    res['HOTA'] = np.sqrt(res['DetA'] * res['AssA'])
    res['OWTA'] = np.sqrt(res['DetRe'] * res['AssA'])
    res['HOTA(0)'] = res['HOTA'][0]
    res['LocA(0)'] = res['LocA'][0]
    res['HOTALocA(0)'] = res['HOTA(0)'] * res['LocA(0)']
    return res


def _empty_result():
    res = {}
    for field in FLOAT_ARRAY_FIELDS + INTEGER_ARRAY_FIELDS:
        res[field] = np.zeros((len(ARRAY_LABELS)), dtype=float)
    for field in FLOAT_FIELDS:
        res[field] = 0
    return res


def one_sided_result(num_gt_dets, num_tracker_dets):
    """`eval_sequence`'s early return: no result detections (checked first), or no ground-truth detections."""
    res = _empty_result()
    if num_tracker_dets == 0:
        res['HOTA_FN'] = num_gt_dets * np.ones((len(ARRAY_LABELS)), dtype=float)
    else:
        assert num_gt_dets == 0
        res['HOTA_FP'] = num_tracker_dets * np.ones((len(ARRAY_LABELS)), dtype=float)
    res['LocA'] = np.ones((len(ARRAY_LABELS)), dtype=float)
    res['LocA(0)'] = 1.0
    return res


def sequence_result(tp_fn_fp, matches, loca_sum, gt_id_count, tracker_id_count):
    """`eval_sequence` after its frame loops, from the tables of one class sequence (hota_counts.HotaTables.of_class)."""
    res = _empty_result()
    res['HOTA_TP'] += tp_fn_fp[:, 0]
    res['HOTA_FN'] += tp_fn_fp[:, 1]
    res['HOTA_FP'] += tp_fn_fp[:, 2]
    res['LocA'] += loca_sum
    gt_id_count = gt_id_count.astype(float)[:, np.newaxis]
    tracker_id_count = tracker_id_count.astype(float)[np.newaxis, :]
    for a in range(len(ARRAY_LABELS)):
        matches_count = matches[a].astype(float)
        ass_a = matches_count / np.maximum(1, gt_id_count + tracker_id_count - matches_count)
        res['AssA'][a] = np.sum(matches_count * ass_a) / np.maximum(1, res['HOTA_TP'][a])
        ass_re = matches_count / np.maximum(1, gt_id_count)
        res['AssRe'][a] = np.sum(matches_count * ass_re) / np.maximum(1, res['HOTA_TP'][a])
        ass_pr = matches_count / np.maximum(1, tracker_id_count)
        res['AssPr'][a] = np.sum(matches_count * ass_pr) / np.maximum(1, res['HOTA_TP'][a])
    res['LocA'] = np.maximum(1e-10, res['LocA']) / np.maximum(1e-10, res['HOTA_TP'])
    return _compute_final_fields(res)


def _combine_sum(all_res, field):
    return sum([all_res[k][field] for k in all_res.keys()])


def _combine_weighted_av(all_res, field, comb_res, weight_field):
    return sum([all_res[k][field] * all_res[k][weight_field] for k in all_res.keys()]) / np.maximum(1.0, comb_res[weight_field])


def combine_sequences(all_res):
    res = {}
    for field in INTEGER_ARRAY_FIELDS:
        res[field] = _combine_sum(all_res, field)
    for field in ['AssRe', 'AssPr', 'AssA']:
        res[field] = _combine_weighted_av(all_res, field, res, weight_field='HOTA_TP')
    loca_weighted_sum = sum([all_res[k]['LocA'] * all_res[k]['HOTA_TP'] for k in all_res.keys()])
    res['LocA'] = np.maximum(1e-10, loca_weighted_sum) / np.maximum(1e-10, res['HOTA_TP'])
    return _compute_final_fields(res)


combine_classes_det_averaged = combine_sequences                    # (the reference states the same lines twice)


def combine_classes_class_averaged(all_res, ignore_empty_classes=False):
    res = {}
    kept = {k: v for k, v in all_res.items()
            if not ignore_empty_classes or (v['HOTA_TP'] + v['HOTA_FN'] + v['HOTA_FP'] > 0 + EPS).any()}
    for field in INTEGER_ARRAY_FIELDS:
        res[field] = _combine_sum(kept, field)
    for field in FLOAT_FIELDS + FLOAT_ARRAY_FIELDS:
        res[field] = np.mean([v[field] for v in kept.values()], axis=0)
    return res


def summary_row(res):
    """The mean over alpha of every summary field (`_summary_row` without its formatting) -> {field: float}."""
    return OrderedDict((h, float(np.mean(res[h])) if h in FLOAT_ARRAY_FIELDS else float(res[h])) for h in SUMMARY_FIELDS)


# ---- one video ----------------------------------------------------------------------------------------------------------------------------
def video_results(gt_area, tr_area, inter, classes):
    """The sequences of one video.  gt_area int32 [G, T], tr_area int32 [D, T], inter int32 [D, G, T] (None where a side has no track);
    classes: [(key, ground-truth indices, track indices)], neither both empty -> {key: res}.  One `hota_counts` call for the classes
    with detections on both sides; the others take the early return."""
    out, both = OrderedDict(), []
    for key, gi, pi in classes:
        n_g = int((gt_area[torch.from_numpy(np.asarray(gi, np.int64))] > 0).sum()) if len(gi) else 0
        n_p = int((tr_area[torch.from_numpy(np.asarray(pi, np.int64))] > 0).sum()) if len(pi) else 0
        if n_p == 0 or n_g == 0:
            out[key] = one_sided_result(n_g, n_p)
        else:
            out[key] = None
            both.append((key, gi, pi))
    if both:
        T = int(gt_area.shape[1])
        gt_starts = np.concatenate([[0], np.cumsum([len(gi) for _, gi, _ in both])])
        tr_starts = np.concatenate([[0], np.cumsum([len(pi) for _, _, pi in both])])
        tables = hota_counts(gt_area, tr_area, inter, np.concatenate([gi for _, gi, _ in both]), gt_starts,
                             np.concatenate([pi for _, _, pi in both]), tr_starts, THRESHOLDS)
        tables = type(tables)(*(x.cpu() for x in tables))            # one download per table, not one per class
        for c, (key, _, _) in enumerate(both):
            out[key] = sequence_result(*tables.of_class(c, gt_starts, tr_starts, T)[:5])
    return out


def hota_from_idmaps(gt, pred, device=None):
    """The result of ONE class-agnostic sequence from id maps: gt, pred int32 [T, H, W], id 0 = background; the ids of a side are its
    tracks, in ascending order.  The areas and overlaps are sums over the pair table of `pair_counts`."""
    gt, pred = torch.as_tensor(gt), torch.as_tensor(pred)
    dev = _device(device, gt)
    gt, pred = gt.to(dev), pred.to(dev)
    gi, pi = torch.unique(gt), torch.unique(pred)
    gi, pi = gi[gi != 0].to(torch.int32), pi[pi != 0].to(torch.int32)
    n_g, n_p = int(gi.numel()), int(pi.numel())
    if n_g == 0 or n_p == 0:
        other = pi if n_g == 0 else gi
        side = pred if n_g == 0 else gt
        dets = int(sum(int((side == int(k)).flatten(1).any(dim=1).sum()) for k in other))
        return one_sided_result(dets if n_p == 0 else 0, dets if n_g == 0 else 0)
    counts = pair_counts(gt, pred, gi, pi)[0].to(torch.int64)       # [T, G + 1, P + 1]; the last row / column: background
    inter = counts[:, :n_g, :n_p].permute(2, 1, 0).to(torch.int32).contiguous()
    gt_area = counts[:, :n_g, :].sum(dim=2).T.to(torch.int32).contiguous()
    tr_area = counts[:, :, :n_p].sum(dim=1).T.to(torch.int32).contiguous()
    return video_results(gt_area, tr_area, inter, [(ALL, np.arange(n_g), np.arange(n_p))])[ALL]


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------------------
class HOTAEvaluator:
    """The ground-truth file (a path or the loaded dictionary), the output directory (`hota-final.txt`, `results.json`), the device of
    the counts, the score threshold and whether classes are ignored.  `process(inputs, outputs)` takes what `YTVISEvaluator.process`
    takes (a driver's output dictionary, or the list of records of ONE OR MORE whole videos) and counts those videos at once; a video
    is processed once.  `evaluate()` scores the videos without results as missed and combines."""

    def __init__(self, gt_json, output_dir=None, device=None, score_thresh=0.0, class_agnostic=False):
        if isinstance(gt_json, (str, os.PathLike)):
            with open(gt_json, "r") as f:
                gt_json = json.load(f)
        assert type(gt_json) == dict, 'annotation file format {} not supported'.format(type(gt_json))
        if gt_json.get("annotations") is None:
            raise ValueError("HOTA needs a ground-truth file with `annotations`")
        self._dataset, self._output_dir, self._device = gt_json, output_dir, _device(device)
        self._score_thresh, self._class_agnostic = float(score_thresh), bool(class_agnostic)
        self._videos = {v["id"]: v for v in gt_json["videos"]}
        self._cat_ids = sorted(c["id"] for c in gt_json["categories"])
        self._cat_names = {c["id"]: c.get("name", str(c["id"])) for c in gt_json["categories"]}
        self._gt_by_video = defaultdict(list)
        for g in gt_json["annotations"]:
            if not g.get("iscrowd", 0):
                self._gt_by_video[g["video_id"]].append(g)
        self.reset()

    def reset(self):
        self._predictions = []
        self.sequences = OrderedDict()                               # (video, class key) -> res
        self._done = set()

    def process(self, inputs, outputs):
        if isinstance(outputs, dict):
            prediction = instances_to_coco_json_video(inputs, outputs)
        elif isinstance(outputs, list):
            prediction = outputs
        else:
            raise ValueError
        assert set(a["video_id"] for a in prediction) <= set(self._videos), 'Results do not correspond to current coco set'
        self._predictions.extend(prediction)
        by_video = defaultdict(list)
        for a in prediction:
            by_video[a["video_id"]].append(a)
        for vid, recs in by_video.items():
            self._count_video(vid, recs)

    def _classes(self, gts, dts):
        if self._class_agnostic:
            return [(ALL, np.arange(len(gts)), np.arange(len(dts)))] if len(gts) or len(dts) else []
        out = []
        for cat in self._cat_ids:
            gi = np.array([i for i, g in enumerate(gts) if g["category_id"] == cat], np.int64)
            pi = np.array([i for i, d in enumerate(dts) if d["category_id"] == cat], np.int64)
            if len(gi) or len(pi):
                out.append((cat, gi, pi))
        return out

    def _count_video(self, vid, recs):
        if vid in self._done:
            raise ValueError(f"video {vid}: processed twice")
        self._done.add(vid)
        video = self._videos[vid]
        H, W = video["height"], video["width"]
        gts = self._gt_by_video.get(vid, [])
        dts = [d for d in recs if d.get("score", 1.0) >= self._score_thresh]
        if len(dts) and "segmentations" not in dts[0]:
            raise ValueError("the results hold no 'segmentations': only mask results are scored")
        T = None
        sides = []
        for anns in (gts, dts):
            if len(anns) == 0:
                sides.append(None)
                continue
            runs, rows, Ts = _video_runs(anns, video)
            if T is not None and Ts != T:
                raise ValueError(f"video {vid}: results of {Ts} frames, annotations of {T}")
            T = Ts
            sides.append((runs, rows))
        if T is None:
            return
        dev = self._device
        area = [torch.zeros((0, T), dtype=torch.int32, device=dev) if s is None else
                s[0].areas().reshape(-1, T)[torch.from_numpy(s[1])].to(torch.int32).to(dev) for s in sides]
        inter = None
        if sides[0] is not None and sides[1] is not None:
            (g_runs, g_rows), (d_runs, d_rows) = sides
            inter = vis_overlap(d_runs.to(dev), g_runs.to(dev), T, H, W)
            inter = inter[torch.from_numpy(d_rows).to(dev)][:, torch.from_numpy(g_rows).to(dev)].contiguous()
        for key, res in video_results(area[0], area[1], inter, self._classes(gts, dts)).items():
            self.sequences[vid, key] = res

    def evaluate(self):
        for vid in sorted(self._videos, key=str):
            if vid not in self._done and len(self._gt_by_video.get(vid, [])):
                self._count_video(vid, [])
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, "results.json"), "w") as f:
                f.write(json.dumps(self._predictions))
        by_class = OrderedDict()
        for key in ([ALL] if self._class_agnostic else self._cat_ids):
            seqs = OrderedDict((v["id"], self.sequences[v["id"], key]) for v in self._dataset["videos"] if (v["id"], key) in self.sequences)
            if seqs:
                by_class[key] = combine_sequences(seqs)
        if not by_class:
            return {}
        out = {"per_class": by_class, "cls_comb_cls_av": combine_classes_class_averaged(by_class),
               "cls_comb_det_av": combine_classes_det_averaged(by_class)}
        out["summary"] = OrderedDict([("cls_comb_cls_av", summary_row(out["cls_comb_cls_av"])),
                                      ("cls_comb_det_av", summary_row(out["cls_comb_det_av"]))] +
                                     [(str(self._cat_names.get(k, k)), summary_row(r)) for k, r in by_class.items()])
        self.last_lines = summary_lines(out["summary"])
        if self._output_dir:
            write_summary(self._output_dir, self.last_lines)
        return out


def summary_lines(summary):
    """One header line and one line per row of the summary, values in percent as TrackEval prints them ({0:1.5g})."""
    lines = ['%-35s' % 'HOTA' + ''.join('%-12s' % h for h in SUMMARY_FIELDS)]
    for name, row in summary.items():
        lines.append('%-35s' % name + ''.join('%-12s' % "{0:1.5g}".format(100 * row[h]) for h in SUMMARY_FIELDS))
    return lines


def write_summary(output_dir, lines):
    os.makedirs(output_dir, exist_ok=True)
    with open(os.path.join(output_dir, "hota-final.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def evaluate_hota_files(gt_json, results_json, output_dir=None, device=None, score_thresh=0.0, class_agnostic=False):
    """The annotation file and the result file (paths, or the loaded dictionary / list) -> what `HOTAEvaluator.evaluate` returns; with
    `output_dir` the summary goes to hota-final.txt there (the result file is not written again)."""
    ev = HOTAEvaluator(gt_json, device=device, score_thresh=score_thresh, class_agnostic=class_agnostic)
    if isinstance(results_json, (str, os.PathLike)):
        with open(results_json, "r") as f:
            results_json = json.load(f)
    assert type(results_json) == list, 'results in not an array of objects'
    ev.process(None, results_json)
    out = ev.evaluate()
    if output_dir and out:
        write_summary(output_dir, ev.last_lines)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="HOTA of a YouTube-VIS-format tracking result file")
    ap.add_argument("--gt_json", required=True, help="the annotation file (YouTube-VIS format, with `annotations`)")
    ap.add_argument("--results", required=True, help="results.json: the list of result records")
    ap.add_argument("--score_thresh", type=float, default=0.0, help="result tracks below this score are dropped")
    ap.add_argument("--class_agnostic", action="store_true", help="one sequence per video, classes ignored")
    ap.add_argument("--output_dir", default=None, help="where hota-final.txt is written (default: beside the result file)")
    ap.add_argument("--device", default=None)
    args = ap.parse_args(argv)
    out = evaluate_hota_files(args.gt_json, args.results, output_dir=args.output_dir or os.path.dirname(os.path.abspath(args.results)), device=args.device, score_thresh=args.score_thresh,
                              class_agnostic=args.class_agnostic)
    for line in summary_lines(out["summary"]) if out else ():
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
