"""VPQ and STQ of a VIPSeg-format result, from one pair table per frame (pair_counts.py) instead of the pixels.

The reference scores a result with `VPSEvaluator.evaluate` (univs/evaluation/vps_evaluation.py:180-424): `vpq_compute_single_core`
(eval_vpq_vps.py:77-234) slides a window of 1, 2, 4, 6 and 8 frames over every video and, for every window, re-opens its PNGs and sorts
nf x H x W keys; `STQuality` (eval_stquality_vps.py) then goes over the pixels again.  Both metrics are additive over frames: they only
need, per frame, how many pixels carry each (ground-truth id, predicted id) pair.  Here that table is counted once per frame on the GPU
and everything else is host arithmetic in float64 over tables:

  vpq_from_tables      `vpq_compute_single_core` + `PQStat.pq_average`: window tables are differences of a running sum; the `iou` terms
                       are added in the reference's order (windows in order, pairs in ascending gt_id 2^24 + pred_id, one sum per video,
                       videos in order), so the sums are the same doubles
  stq_from_tables      `eval_stq_vps.main` + `STQuality` with its parameters (124 classes, ignore 255, shift 16, offset 2^24)
  evaluate_vps_files   the file-level entry point: every PNG read once, one upload and one `pair_counts` call per video, the reference's
                       result files (vpq-<k>.txt, vpq-final.txt, stq-final.txt) in its formatting
  VPSEvaluator         reset / process / evaluate with the reference's call pattern; `process` takes the tables from the int32
                       `pred_masks` it is handed, so `evaluate` never re-reads a predicted PNG

`python -m univs_amd.evaluation.vps --submit_dir ... --truth_dir ... --pan_gt_json_file ...` is the reference's two scripts in one.
Single process: the reference's gather over ranks (vps_evaluation.py:184-190) is left to the caller.
"""
import argparse
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from ._counts import check_reader, device_stack
from .pair_counts import pair_counts

VOID = 0
NFRAMES = (1, 2, 4, 6, 8)                  # eval_vpq_vps.py:414; the file of a length is vpq-<(nframes - 1) * 5>.txt
STQ_CLASSES, STQ_IGNORE, STQ_SHIFT, STQ_OFFSET = 124, 255, 16, 2 ** 24     # eval_stq_vps.py:44-46, :75
_EPSILON = 1e-15


class VideoTables:
    """One video: its annotation records of both JSONs, frame by frame, and its pair tables.  counts int64 [T, G + 1, P + 1] over the
    ascending id tables gt_ids [G] / pred_ids [P] (both hold VOID); first_unknown [T, 2]."""

    def __init__(self, video_id, gt_frames, pred_frames, counts, gt_ids, pred_ids, first_unknown):
        self.video_id, self.gt_frames, self.pred_frames = video_id, gt_frames, pred_frames
        self.counts = np.asarray(counts, dtype=np.int64)
        self.gt_ids, self.pred_ids = np.asarray(gt_ids, dtype=np.int64), np.asarray(pred_ids, dtype=np.int64)
        self.first_unknown = np.asarray(first_unknown, dtype=np.int64)
        T, G1, P1 = self.counts.shape
        if T != len(gt_frames) or G1 != len(self.gt_ids) + 1 or P1 != len(self.pred_ids) + 1:
            raise ValueError(f"{video_id}: tables {self.counts.shape} for {len(gt_frames)} frames, {len(self.gt_ids)} x {len(self.pred_ids)} ids")


def id_table(frames):
    """The ascending id table of a video: VOID and every id its records list."""
    return np.array(sorted({VOID} | {int(el["id"]) for fr in frames for el in fr["segments_info"]}), dtype=np.int64)


def _merged_segments(frame):
    """A frame's segments by id, in the record's order; an id listed twice adds its areas (eval_vpq_vps.py:100-111)."""
    out = OrderedDict()
    for el in frame["segments_info"]:
        if el["id"] in out:
            out[el["id"]]["area"] += el["area"]
        else:
            out[el["id"]] = dict(el)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# VPQ
# ------------------------------------------------------------------------------------------------------------------------------------
class _Stat:
    __slots__ = ("iou", "tp", "fp", "fn")

    def __init__(self):
        self.iou, self.tp, self.fp, self.fn = 0.0, 0, 0, 0


def _checked_pred_frame(v, t, categories):
    """The predicted segments of frame t with their areas taken from the table, after the reference's checks (:112-130)."""
    segs = _merged_segments(v.pred_frames[t])
    area = v.counts[t].sum(axis=0)                                   # per predicted id (the last one: ids that are not listed)
    if area[-1] > 0:
        raise KeyError("Segment with ID {} is presented in PNG and not presented in JSON.".format(int(v.first_unknown[t, 1])))
    left = set(el["id"] for el in v.pred_frames[t]["segments_info"])
    for p in np.nonzero(area[:-1])[0]:
        label, cnt = int(v.pred_ids[p]), int(area[p])
        if label not in segs:
            if label == VOID:
                continue
            raise KeyError("Segment with ID {} is presented in PNG and not presented in JSON.".format(label))
        if "area" in segs[label]:
            assert segs[label]["area"] == cnt, f"Mismatch numbers of {segs[label]['area']} and {cnt}"
        segs[label]["area"] = cnt
        left.remove(label)
        if segs[label]["category_id"] not in categories:
            raise KeyError("Segment with ID {} has unknown category_id {}.".format(label, segs[label]["category_id"]))
    if left:
        raise KeyError("The following segment IDs {} are presented in JSON and not presented in PNG.".format(list(left)))
    return segs


def _tube(frames):
    """Per-frame segment dicts -> the window's: the first frame that lists an id gives its category and crowd flag, areas add (:141-153)."""
    out = OrderedDict()
    for segs in frames:
        for k, s in segs.items():
            if k not in out:
                out[k] = dict(s)
            else:
                out[k]["area"] += s["area"]
    return out


def _vpq_video(v, categories, nframes, stat):
    T = len(v.gt_frames)
    if T - nframes + 1 <= 0:
        return
    pred_frames = [_checked_pred_frame(v, t, categories) for t in range(T)]
    gt_frames = [_merged_segments(fr) for fr in v.gt_frames]
    G, P = len(v.gt_ids), len(v.pred_ids)
    gpos = {int(i): k for k, i in enumerate(v.gt_ids)}
    ppos = {int(i): k for k, i in enumerate(v.pred_ids)}
    void_row = gpos[VOID]
    running = np.concatenate([np.zeros((1,) + v.counts.shape[1:], np.int64), np.cumsum(v.counts, axis=0)])
    video = {}                                                       # this video's sums; added to `stat` at the end, as `vpq_stat += tmp`

    def cat_stat(c):
        if c not in video:
            video[c] = _Stat()
        return video[c]
    for idx in range(T - nframes + 1):
        tube = running[idx + nframes] - running[idx]                 # [G + 1, P + 1]
        gt_segs = _tube(gt_frames[idx:idx + nframes])
        pred_segs = _tube(pred_frames[idx:idx + nframes])
        rows = tube.sum(axis=1)
        for gid, s in gt_segs.items():                               # the area of an id that occurs is recounted from the pixels (:162-164)
            if rows[gpos[gid]] > 0:
                s["area"] = int(rows[gpos[gid]])
        gt_matched, pred_matched = set(), set()
        gs, ps = np.nonzero(tube[:G, :P])                            # row-major: ascending gt_id 2^24 + pred_id
        for g, p in zip(gs.tolist(), ps.tolist()):
            gt_label, pred_label = int(v.gt_ids[g]), int(v.pred_ids[p])
            if gt_label not in gt_segs or pred_label not in pred_segs:
                continue
            gseg, pseg = gt_segs[gt_label], pred_segs[pred_label]
            if gseg["iscrowd"] == 1 or gseg["category_id"] != pseg["category_id"]:
                continue
            inter = int(tube[g, p])
            union = int(pseg["area"]) + int(gseg["area"]) - inter - int(tube[void_row, p])
            iou = inter / union
            assert iou <= 1.0, f"INVALID IOU VALUE: {iou} on the gt_label {gt_label} and the pred_label {pred_label}"
            if iou > 0.5:
                st = cat_stat(gseg["category_id"])
                st.tp += 1
                st.iou += iou
                gt_matched.add(gt_label)
                pred_matched.add(pred_label)
        crowd_of = {}
        for gt_label, s in gt_segs.items():
            if gt_label in gt_matched:
                continue
            if s["iscrowd"] == 1:
                crowd_of[s["category_id"]] = gt_label
                continue
            cat_stat(s["category_id"]).fn += 1
        for pred_label, s in pred_segs.items():
            if pred_label in pred_matched:
                continue
            p = ppos[pred_label]
            ignored = int(tube[void_row, p])
            if s["category_id"] in crowd_of:
                ignored += int(tube[gpos[crowd_of[s["category_id"]]], p])
            if ignored / int(s["area"]) > 0.5:                       # mostly on VOID and its category's crowd region
                continue
            cat_stat(s["category_id"]).fp += 1
    for c, st in video.items():
        tot = stat.setdefault(c, _Stat())
        tot.iou += st.iou
        tot.tp += st.tp
        tot.fp += st.fp
        tot.fn += st.fn


def _pq_average(stat, categories, isthing):
    pq, sq, rq, n = 0, 0, 0, 0
    per_class = OrderedDict()
    for label, info in categories.items():
        if isthing is not None and isthing != (info["isthing"] == 1):
            continue
        st = stat.get(label) or _Stat()
        if st.tp + st.fp + st.fn == 0:
            per_class[label] = {"pq": 0.0, "sq": 0.0, "rq": 0.0, "iou": 0.0, "tp": 0, "fp": 0, "fn": 0}
            continue
        n += 1
        pq_c = st.iou / (st.tp + 0.5 * st.fp + 0.5 * st.fn)
        sq_c = st.iou / st.tp if st.tp != 0 else 0
        rq_c = st.tp / (st.tp + 0.5 * st.fp + 0.5 * st.fn)
        per_class[label] = {"pq": pq_c, "sq": sq_c, "rq": rq_c, "iou": st.iou, "tp": st.tp, "fp": st.fp, "fn": st.fn}
        pq += pq_c
        sq += sq_c
        rq += rq_c
    return {"pq": pq / n, "sq": sq / n, "rq": rq / n, "n": n}, per_class


def vpq_text(result):
    """The text of vpq-<k>.txt (eval_vpq_vps.py:299-308)."""
    lines = ["================================================\n",
             "{:10s}| {:>5s}  {:>5s}  {:>5s} {:>5s}".format("", "PQ", "SQ", "RQ", "N\n"),
             "-" * (10 + 7 * 4) + "\n"]
    for name in ("All", "Things", "Stuff"):
        r = result[name]
        lines.append("{:10s}| {:5.1f}  {:5.1f}  {:5.1f} {:5d}\n".format(name, 100 * r["pq"], 100 * r["sq"], 100 * r["rq"], r["n"]))
    lines.append("{:4s}| {:>5s} {:>5s} {:>5s} {:>6s} {:>7s} {:>7s} {:>7s}\n".format("IDX", "PQ", "SQ", "RQ", "IoU", "TP", "FP", "FN"))
    for idx, r in result["per_class"].items():
        lines.append("{:4d} | {:5.1f} {:5.1f} {:5.1f} {:6.1f} {:7d} {:7d} {:7d}\n".format(idx, 100 * r["pq"], 100 * r["sq"], 100 * r["rq"],
                                                                                        r["iou"], r["tp"], r["fp"], r["fn"]))
    return "".join(lines)


def vpq_from_tables(videos, categories, nframes_list=NFRAMES):
    """{nframes: {"All" / "Things" / "Stuff": {"pq", "sq", "rq", "n"}, "per_class": {category id: {"pq", "sq", "rq", "iou", "tp", "fp",
    "fn"}}}} and, under "final", the means over the window lengths of 100 PQ ({"vpq_all", "vpq_thing", "vpq_stuff"}).  `videos`:
    VideoTables in the ground truth's order; `categories`: {category id: its record of the ground-truth JSON}, in the JSON's order."""
    out = OrderedDict()
    for nframes in nframes_list:
        stat = {}
        for v in videos:
            _vpq_video(v, categories, nframes, stat)
        res = {}
        for name, isthing in (("All", None), ("Things", True), ("Stuff", False)):
            res[name], per_class = _pq_average(stat, categories, isthing)
            if name == "All":
                res["per_class"] = per_class
        out[nframes] = res
    alls = [100 * out[n]["All"]["pq"] for n in nframes_list]
    things = [100 * out[n]["Things"]["pq"] for n in nframes_list]
    stuffs = [100 * out[n]["Stuff"]["pq"] for n in nframes_list]
    out["final"] = {"vpq_all": sum(alls) / len(alls), "vpq_thing": sum(things) / len(things), "vpq_stuff": sum(stuffs) / len(stuffs)}
    return out


def vpq_final_text(final):
    return "vpq_all:%.4f\n" % final["vpq_all"] + "vpq_thing:%.4f\n" % final["vpq_thing"] + "vpq_stuff:%.4f\n" % final["vpq_stuff"]


# ------------------------------------------------------------------------------------------------------------------------------------
# STQ
# ------------------------------------------------------------------------------------------------------------------------------------
def _first_seen(frames):
    """id -> its position in the video's first-seen list (eval_stq_vps.py:114-132): the instance number the reference paints."""
    num = {}
    for fr in frames:
        for el in fr["segments_info"]:
            if el["id"] not in num:
                num[el["id"]] = len(num)
    return num


def _painted_labels(frame, ids, num):
    """Per table index (the last: ids that are not listed) the label the reference paints on that id's pixels in this frame:
    (category << 16) + instance number, (255 << 16) + 255 for an id the frame's record does not list (:140-158)."""
    lab = np.full(len(ids) + 1, (STQ_IGNORE << STQ_SHIFT) + STQ_IGNORE, dtype=np.int64)
    pos = {int(i): k for k, i in enumerate(ids)}
    for el in frame["segments_info"]:
        lab[pos[el["id"]]] = (int(el["category_id"]) << STQ_SHIFT) + num[el["id"]]
    return lab


def _add(d, key, count):
    if key in d:
        d[key] += count
    else:
        d[key] = count


def stq_from_tables(videos, categories, num_classes=STQ_CLASSES, ignore_label=STQ_IGNORE):
    """{"STQ", "AQ", "IoU", "STQ_per_seq", "AQ_per_seq", "IoU_per_seq", "ID_per_seq", "Length_per_seq"} as `STQuality.result()` after
    `eval_stq_vps.main`'s updates.  `categories`: the ground-truth JSON's list (or dict) of category records."""
    cats = list(categories.values()) if isinstance(categories, dict) else list(categories)
    things = np.array([c["id"] for c in cats if c["isthing"]], dtype=np.int64)
    bit_mask = (1 << STQ_SHIFT) - 1
    size = num_classes + 1 if ignore_label >= num_classes else num_classes
    include = np.arange(num_classes) if ignore_label >= num_classes else np.array([i for i in range(num_classes) if i != ignore_label])
    confusions, preds_all, gts_all, inters_all, lengths = [], [], [], [], []
    for v in videos:
        if len(v.gt_frames) == 0:
            continue
        confusion = np.zeros((size, size), dtype=np.int64)
        preds, gts, inters = OrderedDict(), OrderedDict(), OrderedDict()
        gnum, pnum = _first_seen(v.gt_frames), _first_seen(v.pred_frames)
        for t in range(len(v.gt_frames)):
            glab, ginv = np.unique(_painted_labels(v.gt_frames[t], v.gt_ids, gnum), return_inverse=True)
            plab, pinv = np.unique(_painted_labels(v.pred_frames[t], v.pred_ids, pnum), return_inverse=True)
            M = np.zeros((len(glab), len(plab)), dtype=np.int64)     # the frame's table by painted label
            np.add.at(M, (ginv.reshape(-1)[:, None], pinv.reshape(-1)[None, :]), v.counts[t])
            gsem, psem = glab >> STQ_SHIFT, plab >> STQ_SHIFT
            if ignore_label > num_classes:
                gsem = np.where(gsem != ignore_label, gsem, num_classes)
                psem = np.where(psem != ignore_label, psem, num_classes)
            np.add.at(confusion, (gsem[:, None], psem[None, :]), M)
            g_thing, p_thing = np.isin(gsem, things), np.isin(psem, things)
            crowd = g_thing & ((glab & bit_mask) == 0)               # instance number 0 of a thing class counts as crowd
            g_keep = g_thing & ~crowd
            pred_area = M[~crowd].sum(axis=0)
            for p in np.nonzero(p_thing & (pred_area > 0))[0]:
                _add(preds, int(plab[p]), int(pred_area[p]))
            gt_area = M.sum(axis=1)
            for g in np.nonzero(g_keep & (gt_area > 0))[0]:
                _add(gts, int(glab[g]), int(gt_area[g]))
            both = M * (g_keep[:, None] & p_thing[None, :])
            for g, p in zip(*np.nonzero(both)):
                _add(inters, int(glab[g]) * STQ_OFFSET + int(plab[p]), int(both[g, p]))
        confusions.append(confusion)
        preds_all.append(preds)
        gts_all.append(gts)
        inters_all.append(inters)
        lengths.append(len(v.gt_frames))

    n = len(gts_all)
    num_tubes, aq_per_seq, iou_per_seq = [0] * n, [0] * n, [0] * n
    for i in range(n):
        outer = 0.0
        for gt_id, gt_size in gts_all[i].items():
            inner = 0.0
            for pr_id, pr_size in preds_all[i].items():
                tpa = inters_all[i].get(STQ_OFFSET * gt_id + pr_id)
                if tpa is not None:
                    inner += tpa * (tpa / (tpa + (pr_size - tpa) + (gt_size - tpa)))
            outer += 1.0 / gt_size * inner
        num_tubes[i] = len(gts_all[i])
        aq_per_seq[i] = outer
    aq_mean = np.sum(aq_per_seq) / np.maximum(np.sum(num_tubes), _EPSILON)
    aq_per_seq = aq_per_seq / np.maximum(num_tubes, _EPSILON)

    def mean_iou(c, eps):
        tp = c.diagonal()
        unions = tp + (c.sum(axis=0) - tp) + (c.sum(axis=1) - tp)
        ious = tp.astype(np.double) / np.maximum(unions, eps).astype(np.double)
        return np.sum(ious) / np.count_nonzero(unions)
    total = np.zeros((size, size), dtype=np.int64)
    keep = np.zeros((size, size), dtype=np.int64)
    keep[include, :] = 1                                             # the ignore row out: no false positives against void
    for i, c in enumerate(confusions):
        c = c * keep
        total += c
        iou_per_seq[i] = mean_iou(c, 1e-15)
    iou_mean = mean_iou(total, _EPSILON)
    return {"STQ": np.sqrt(aq_mean * iou_mean), "AQ": aq_mean, "IoU": float(iou_mean), "STQ_per_seq": np.sqrt(aq_per_seq * iou_per_seq),
            "AQ_per_seq": aq_per_seq, "IoU_per_seq": iou_per_seq, "ID_per_seq": list(range(n)), "Length_per_seq": lengths}


def stq_text(result):
    """The text of stq-final.txt (eval_stq_vps.py:165-167: no line breaks)."""
    return "STQ : {}".format(result["STQ"]) + "AQ :{}".format(result["AQ"]) + "IoU:{}".format(result["IoU"])


# ------------------------------------------------------------------------------------------------------------------------------------
# tables of a video, and the file-level entry points
# ------------------------------------------------------------------------------------------------------------------------------------
def _read_rgb(path):
    from PIL import Image
    with Image.open(path) as im:
        size = im.size
        return np.array(im if im.mode == "RGB" else im.convert("RGB")), size


def _read_stack(paths):
    frames = [_read_rgb(p)[0] for p in paths]
    return np.stack(frames) if frames else np.zeros((0, 1, 1, 3), np.uint8)


def video_tables(video_id, gt_frames, pred_frames, gt_map, pred_map, device=None):
    """VideoTables of one video from its two maps (numpy or torch; uint8 [T, H, W, 3] or int32 [T, H, W]): one upload, one `pair_counts`."""
    gt_ids, pred_ids = id_table(gt_frames), id_table(pred_frames)
    T = len(gt_frames)
    if T == 0:
        return VideoTables(video_id, gt_frames, pred_frames, np.zeros((0, len(gt_ids) + 1, len(pred_ids) + 1)), gt_ids, pred_ids, np.zeros((0, 2)))
    device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    g = torch.as_tensor(gt_map).to(device)
    p = torch.as_tensor(pred_map).to(device)
    counts, unknown = pair_counts(g, p, torch.from_numpy(gt_ids), torch.from_numpy(pred_ids))
    return VideoTables(video_id, gt_frames, pred_frames, counts.cpu().numpy(), gt_ids, pred_ids, unknown.cpu().numpy())


def _by_video(jsons):
    return {a["video_id"]: a["annotations"] for a in jsons["annotations"]}


def _tables_from_files(video, gt_frames, pred_frames, submit_dir, truth_dir, device, reader="host"):
    """reader "gpu": both sides are decoded on the device as RGB, one call each (`_counts.device_stack`); a video with a file that is
    missing, of another size or not decoded there goes through the loop below, which raises what it raises today."""
    vid = video["video_id"]
    names = [im["file_name"] for im in video["images"]]
    gt_paths = [os.path.join(truth_dir, vid, n) for n in names]
    pred_paths = [os.path.join(submit_dir, "pan_pred", vid, n) for n in names]
    n = len(gt_frames)
    g = device_stack(gt_paths, reader, device, rgb=True)
    p = device_stack(pred_paths, reader, device, rgb=True) if g is not None else None
    if p is not None and g.shape == p.shape:
        return video_tables(vid, gt_frames, pred_frames, g[:n] if n else None, p[:n] if n else None, device)
    gt, pred = [], []
    for gp, pp in zip(gt_paths, pred_paths):
        (g, gsize), (p, psize) = _read_rgb(gp), _read_rgb(pp)
        assert gsize == psize, f"Dismatch shape {gsize} and {psize}"
        gt.append(g)
        pred.append(p)
    return video_tables(vid, gt_frames, pred_frames, np.stack(gt[:n]) if n else None, np.stack(pred[:n]) if n else None, device)


def score_tables(videos, gt_jsons, output_dir=None):
    """VPQ and STQ of the videos' tables, the reference's result files into `output_dir`, and the numbers:
    {"vpq": vpq_from_tables(...), "stq": stq_from_tables(...), "files": {file name: text}}."""
    categories = OrderedDict((el["id"], el) for el in gt_jsons["categories"])
    files = OrderedDict()

    def emit(name, text):
        files[name] = text
        if output_dir:
            os.makedirs(output_dir, exist_ok=True)
            with open(os.path.join(output_dir, name), "w") as f:
                f.write(text)
    vpq = vpq_from_tables(videos, categories)
    for nframes in NFRAMES:
        emit("vpq-%d.txt" % ((nframes - 1) * 5), vpq_text(vpq[nframes]))
    emit("vpq-final.txt", vpq_final_text(vpq["final"]))
    stq = stq_from_tables(videos, gt_jsons["categories"])
    emit("stq-final.txt", stq_text(stq))
    return {"vpq": vpq, "stq": stq, "files": files}


def _collect(gt_jsons, pred_jsons, tables_of):
    """VideoTables of every ground-truth video that has a prediction, in the ground truth's order (eval_vpq_vps.py:376-407).
    A video without one is skipped by VPQ and is a KeyError of STQ (eval_stq_vps.py:98): raised here once VPQ's order allows."""
    gt_j, pred_j = _by_video(gt_jsons), _by_video(pred_jsons)
    videos, missing = [], None
    for video in gt_jsons["videos"]:
        vid = video["video_id"]
        if vid not in pred_j:
            print(f"{vid} does not in prediced json, please double check!!")
            missing = missing or vid
            continue
        assert len(gt_j[vid]) == len(pred_j[vid])
        videos.append(tables_of(video, gt_j[vid], pred_j[vid]))
    return videos, missing


def evaluate_vps_files(submit_dir, truth_dir, pan_gt_json_file, device=None, output_dir=None, reader="host"):
    """`VPSEvaluator.evaluate_vpq` + `evaluate_stq` on a result directory (`pred.json`, `pan_pred/<video>/<frame>.png`): reads every PNG
    once, counts the pair tables of a video with one `pair_counts` call on `device` (default: the GPU when there is one), writes the
    reference's result files into `output_dir` (default: `submit_dir`) and returns `score_tables`' dict.  reader "gpu": the PNGs are
    decoded on the device instead of by Pillow."""
    check_reader(reader)
    with open(os.path.join(submit_dir, "pred.json")) as f:
        pred_jsons = json.load(f)
    with open(pan_gt_json_file) as f:
        gt_jsons = json.load(f)
    videos, missing = _collect(gt_jsons, pred_jsons, lambda video, g, p: _tables_from_files(video, g, p, submit_dir, truth_dir, device,
                                                                                             reader))
    return _score_or_raise(videos, missing, gt_jsons, output_dir or submit_dir)


def _score_or_raise(videos, missing, gt_jsons, output_dir):
    if missing is not None:                                          # VPQ's files first, then STQ's KeyError, as the reference
        categories = OrderedDict((el["id"], el) for el in gt_jsons["categories"])
        vpq = vpq_from_tables(videos, categories)
        os.makedirs(output_dir, exist_ok=True)
        for nframes in NFRAMES:
            with open(os.path.join(output_dir, "vpq-%d.txt" % ((nframes - 1) * 5)), "w") as f:
                f.write(vpq_text(vpq[nframes]))
        with open(os.path.join(output_dir, "vpq-final.txt"), "w") as f:
            f.write(vpq_final_text(vpq["final"]))
        raise KeyError(missing)
    return score_tables(videos, gt_jsons, output_dir)


class VPSEvaluator:
    """The reference's `VPSEvaluator` (vps_evaluation.py) with explicit arguments in place of detectron2's MetadataCatalog:
    `categories` {category id: {"id", "isthing", "color"}} (the metadata's, for the result PNGs' colours), the ground truth's
    `pan_gt_json_file` and `truth_dir` (<truth_dir>/<video>/<frame>.png), and `output_dir`.

    `process` writes the video's PNGs and collects its `pred.json` record through `results.write_vps_predictions`, unchanged.  When the
    video's ground-truth PNGs are there it also counts the video's pair tables at once, from the int32 `pred_masks` it was handed: the
    table's columns are moved from segment ids to the colour ids of the record it just wrote.  `evaluate` then reads no predicted PNG."""

    def __init__(self, categories, pan_gt_json_file, truth_dir, output_dir, device=None, png="host", reader="host"):
        self.categories, self.pan_gt_json_file, self.truth_dir, self._output_dir, self.device = categories, pan_gt_json_file, truth_dir, output_dir, device
        self._gt_jsons = None
        self.png = png                                               # ("host" | "gpu": who compresses the PNGs, results.py)
        self.reader = check_reader(reader)                           # ("host" | "gpu": who decodes them, _counts.device_stack)
        self.reset()

    def _gt(self):
        if self._gt_jsons is None:
            with open(self.pan_gt_json_file) as f:
                self._gt_jsons = json.load(f)
        return self._gt_jsons

    def reset(self):
        self._predictions, self._tables = [], {}
        os.makedirs(os.path.join(self._output_dir, "pan_pred"), exist_ok=True)

    def process(self, inputs, outputs):
        from ..inference.results import write_vps_predictions
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        record = write_vps_predictions(inputs[0], outputs, self._output_dir, self.categories, png=self.png)
        self._predictions.append(record)
        tables = self._tables_in_process(record, outputs)
        if tables is not None:
            self._tables[record["video_id"]] = tables

    def _tables_in_process(self, record, outputs):
        gt_jsons, vid = self._gt(), record["video_id"]
        video = next((v for v in gt_jsons["videos"] if v["video_id"] == vid), None)
        gt_frames = _by_video(gt_jsons).get(vid)
        pred_frames = record["annotations"]
        if video is None or gt_frames is None or len(gt_frames) != len(pred_frames) or len(video["images"]) < len(gt_frames):
            return None
        names = [im["file_name"] for im in video["images"]][:len(gt_frames)]
        if names != [a["file_name"].split(".")[0] + ".png" for a in pred_frames]:
            return None                                              # evaluate() would read other files than the ones just written
        gt_paths = [os.path.join(self.truth_dir, vid, n) for n in names]
        if not all(os.path.exists(p) for p in gt_paths):
            return None
        pan = outputs["pred_masks"]
        pan = pan if isinstance(pan, torch.Tensor) else torch.as_tensor(np.asarray(pan))
        gt = device_stack(gt_paths, self.reader, self.device, rgb=True)
        gt = _read_stack(gt_paths) if gt is None else gt
        if tuple(gt.shape[:3]) != tuple(pan.shape):
            return None                                              # (evaluate() raises the reference's size assertion from the files)
        seg_ids = np.array(sorted({VOID} | {int(s["id"]) for s in outputs["segments_infos"]}), dtype=np.int64)
        gt_ids = id_table(gt_frames)
        device = torch.device(self.device) if self.device is not None else (pan.device if pan.is_cuda else torch.device(
            "cuda" if torch.cuda.is_available() else "cpu"))
        counts, unknown = pair_counts(torch.as_tensor(gt).to(device), pan.to(device=device, dtype=torch.int32),
                                      torch.from_numpy(gt_ids), torch.from_numpy(seg_ids))
        counts, unknown = counts.cpu().numpy().astype(np.int64), unknown.cpu().numpy().astype(np.int64)
        # segment id -> colour id: the record lists, per frame, the segments that have pixels there, in `segments_infos`' order
        # (results.write_vps_predictions' `annotations.append`).  The record's areas check the replay: an entry whose area is not its
        # segment's pixel count, or a segment under two colours, sends the video to the files instead of mis-assigning a column.
        spos = {int(s): k for k, s in enumerate(seg_ids)}
        area = counts.sum(axis=1)                                    # [T, S + 1]
        colour = {}
        for t, ann in enumerate(pred_frames):
            here = [int(s["id"]) for s in outputs["segments_infos"] if area[t, spos[int(s["id"])]] > 0]
            if len(here) != len(ann["segments_info"]):
                return None
            for s, el in zip(here, ann["segments_info"]):
                if int(el["area"]) != int(area[t, spos[s]]) or colour.setdefault(s, int(el["id"])) != int(el["id"]):
                    return None
        pred_ids = id_table(pred_frames)
        ppos = {int(c): k for k, c in enumerate(pred_ids)}
        out = np.zeros(counts.shape[:2] + (len(pred_ids) + 1,), dtype=np.int64)
        for k in range(counts.shape[2]):                             # a pixel of no listed segment is painted VOID by the writer
            c = colour.get(int(seg_ids[k]), VOID) if k < len(seg_ids) else VOID
            out[:, :, ppos[c]] += counts[:, :, k]
        unknown[:, 1] = -1
        return VideoTables(vid, gt_frames, pred_frames, out, gt_ids, pred_ids, unknown)

    def evaluate(self):
        from ..inference.results import write_vps_json
        if len(self._predictions) == 0:
            return {}
        write_vps_json(self._predictions, self._output_dir)
        gt_jsons = self._gt()

        def tables_of(video, g, p):
            t = self._tables.get(video["video_id"])
            return t if t is not None else _tables_from_files(video, g, p, self._output_dir, self.truth_dir, self.device, self.reader)
        videos, missing = _collect(gt_jsons, {"annotations": self._predictions}, tables_of)
        return _score_or_raise(videos, missing, gt_jsons, self._output_dir)


def main(argv=None):
    ap = argparse.ArgumentParser(description="VPQ and STQ of a VIPSeg-format result directory")
    ap.add_argument("--submit_dir", "-i", required=True, help="the result directory: pred.json and pan_pred/<video>/<frame>.png")
    ap.add_argument("--truth_dir", default="datasets/vipseg/VIPSeg_720P/panomasksRGB", help="<truth_dir>/<video>/<frame>.png")
    ap.add_argument("--pan_gt_json_file", default="datasets/vipseg/VIPSeg_720P/panoptic_gt_VIPSeg_val.json")
    ap.add_argument("--device", default=None, help="cuda / cpu (default: the GPU when there is one)")
    ap.add_argument("--reader", default="host", choices=("host", "gpu"), help="who decodes the PNGs: Pillow on the host, or the device")
    a = ap.parse_args(argv)
    r = evaluate_vps_files(a.submit_dir, a.truth_dir, a.pan_gt_json_file, a.device, reader=a.reader)
    print(r["files"]["vpq-final.txt"], end="")
    print("STQ : {}\nAQ :{}\nIoU:{}".format(r["stq"]["STQ"], r["stq"]["AQ"], r["stq"]["IoU"]))
    return r


if __name__ == "__main__":
    main()
