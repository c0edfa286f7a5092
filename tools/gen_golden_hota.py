"""Golden fixtures of the HOTA scoring (tests/golden/g34_hota_*.npz): the reference's own `HOTA` class (univs/evaluation/eval_hota.py over
_base_metric.py: `eval_sequence`, `combine_sequences`, `combine_classes_class_averaged`, `combine_classes_det_averaged`), run unmodified
on small synthetic annotation and result sets.  The file needs `np.float`, which numpy 2 no longer has: the alias is set here, before the
import, and nowhere else.

The reference has no dataset class, so this script builds the `data` dictionary of every (video, class) sequence by the protocol of
univs_amd/evaluation/hota.py, but from the dense boolean masks and not from the run-length codes: crowd ground truths and result tracks
below the score threshold dropped, an id present where its mask is not None and not empty, similarity I / (A_g + A_p - I) in float64.

Each fixture holds the annotation and result JSON as strings (`gt_json`, `results_json`), `score_thresh`, `class_agnostic`, and for a
scored scene the reference's dictionaries, one array per field: `seq__<video>__<class>__<field>`, `cls__<class>__<field>`,
`cls_av__<field>`, `det_av__<field>`; `seq_keys` and `cls_keys` list the sequences and classes in order.  An error scene holds the
exception's type name and text (`error`, `error_text`): the protocol's own sentences, the reference has none.

Margins.  The recorded numbers are functions of each frame's assignment.  Where two assignments of positive pairs reach the same total,
both are HOTA-valid and two solvers may differ, so every scipy call of the reference is wrapped: for every matched pair of positive
score the pair is forbidden and the problem solved again; the drop of the optimal total has to exceed 1e-9 in every frame, or the scene
is built again from the next seed.

Scenes: `clean` (2 videos, 2 classes, a crowd ground truth, a track below the score threshold of 0.3); `more_tracks_than_gt` and
`more_gt_than_tracks` (both orientations of the assignment); `one_by_one`; `t1` (one frame); `empty_frames` (frames without ground
truth, without tracks, without either); `enter_leave` (None masks and empty masks, class-agnostic); `exact_fractions` (IoUs of exactly
1/2, 1/4, 3/4, 1/5, 19/20, on the alpha - eps comparison); `all_zero_frame` (present ids, no overlap); `full_64x64` (64 ids on both sides,
64 x 96 plane); `multi_class` (three categories, one absent from the results, one from the ground truth); `no_tracks`, `no_gt` (the early
returns); `err_size_mismatch`, `err_unknown_video`.

    python tools/gen_golden_hota.py     # needs the reference tree (dev container only)
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
from oracle.ref_harness import REF_ROOT, _pkg  # noqa: E402  (UNIVS_REFERENCE_ROOT)
from univs_amd.inference.results import rle_encode_masks  # noqa: E402

MARGIN = 1e-9


class Tie(Exception):
    pass


# ------------------------------------------------------------------------------------------------------------------------------------
# synthetic annotation and result sets; the dense masks travel beside the records under "_masks" / "_none" and are dropped before dumping
# ------------------------------------------------------------------------------------------------------------------------------------
def boxes(T, H, W, y0, x0, h, w, vy=0, vx=0):
    """bool [T, H, W]: the box [y0, y0 + h) x [x0, x0 + w) moving by (vy, vx) per frame, clipped to the plane."""
    out = np.zeros((T, H, W), bool)
    for t in range(T):
        ya, xa = int(round(y0 + vy * t)), int(round(x0 + vx * t))
        out[t, max(ya, 0):max(ya + h, 0), max(xa, 0):max(xa + w, 0)] = True
    return out


def enc(masks, none_at=()):
    rles = rle_encode_masks(torch.from_numpy(masks))
    return [None if t in none_at else r for t, r in enumerate(rles)], [None if t in none_at else int(m.sum()) for t, m in enumerate(masks)]


def video(vid, T, H, W):
    return {"id": vid, "height": H, "width": W, "length": T, "file_names": ["v%d/%05d.jpg" % (vid, t) for t in range(T)]}


def gt(aid, vid, cat, masks, iscrowd=0, none_at=()):
    segs, areas = enc(masks, none_at)
    return {"id": aid, "video_id": vid, "category_id": cat, "iscrowd": iscrowd, "segmentations": segs, "areas": areas, "_masks": masks,
            "_none": tuple(none_at)}


def det(vid, cat, score, masks, none_at=()):
    segs, _ = enc(masks, none_at)
    return {"video_id": vid, "score": score, "category_id": cat, "segmentations": segs, "height": masks.shape[1], "width": masks.shape[2],
            "_masks": masks, "_none": tuple(none_at)}


def cats(n):
    return [{"id": k + 1, "name": ("person", "dog", "car", "bird")[k]} for k in range(n)]


def random_tracks(rng, vid, cat, T, H, W, G, P, aid=1):
    """G moving boxes as ground truth; P tracks: jittered copies of the first min(G, P) and boxes of their own beyond."""
    anns, res, shapes = [], [], []
    for k in range(G):
        h, w = int(rng.integers(4, 9)), int(rng.integers(4, 10))
        s = (int(rng.integers(0, H - h)), int(rng.integers(0, W - w)), h, w, float(rng.uniform(-1, 1)), float(rng.uniform(-1.5, 1.5)))
        shapes.append(s)
        anns.append(gt(aid + k, vid, cat, boxes(T, H, W, *s)))
    for k in range(P):
        if k < G:
            y0, x0, h, w, vy, vx = shapes[k]
            j = rng.integers(-2, 3, 4)
            s = (y0 + int(j[0]), x0 + int(j[1]), max(h + int(j[2]), 2), max(w + int(j[3]), 2), vy, vx)
        else:
            h, w = int(rng.integers(3, 8)), int(rng.integers(3, 8))
            s = (int(rng.integers(0, H - h)), int(rng.integers(0, W - w)), h, w, float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)))
        res.append(det(vid, cat, float(rng.uniform(0.35, 0.95)), boxes(T, H, W, *s)))
    return anns, res


def scene_clean(seed):
    rng = np.random.default_rng(100 + seed)
    H, W = 24, 32
    frames = {1: 5, 2: 4}
    anns, res, aid = [], [], 1
    for vid, T in frames.items():
        for cat, (G, P) in ((1, (3, 4)), (2, (2, 2))):
            a, r = random_tracks(rng, vid, cat, T, H, W, G, P, aid)
            aid += G
            anns += a
            res += r
    anns.append(gt(aid, 1, 1, boxes(5, H, W, 2, 2, 20, 28), iscrowd=1))              # dropped by the protocol
    res.append(det(1, 1, 0.1, anns[0]["_masks"]))                                    # a perfect track below the threshold: dropped
    return {"videos": [video(v, T, H, W) for v, T in frames.items()], "categories": cats(2), "annotations": anns}, res, {"score_thresh": 0.3}


def _single(seed, G, P, T, H=24, W=32):
    rng = np.random.default_rng(1000 * G + 10 * P + T + 7919 * seed)
    anns, res = random_tracks(rng, 1, 1, T, H, W, G, P)
    return {"videos": [video(1, T, H, W)], "categories": cats(1), "annotations": anns}, res, {}


def scene_more_tracks_than_gt(seed):
    return _single(seed, 3, 7, 6)


def scene_more_gt_than_tracks(seed):
    return _single(seed, 7, 3, 6)


def scene_one_by_one(seed):
    return _single(seed, 1, 1, 4)


def scene_t1(seed):
    return _single(seed, 3, 4, 1)


def scene_empty_frames(seed):
    """T = 7: frame 1 without ground truth, frame 3 without tracks, frame 5 without either."""
    ann, res, _ = _single(seed, 3, 4, 7)
    for a in ann["annotations"]:
        a.update(gt(a["id"], 1, 1, a["_masks"], none_at=(1, 5)))
    for i, r in enumerate(res):
        res[i] = det(1, 1, r["score"], r["_masks"], none_at=(3, 5))
    return ann, res, {}


def scene_enter_leave(seed):
    """Ids that enter and leave: None masks on both sides, and masks that are there but empty.  Class-agnostic."""
    rng = np.random.default_rng(300 + seed)
    T, H, W = 8, 24, 32
    anns, res = random_tracks(rng, 1, 1, T, H, W, 4, 5)
    gone = {0: (0, 1), 1: (6, 7), 2: (3,), 3: ()}
    for k, a in enumerate(anns):
        m = a["_masks"].copy()
        if k == 3:
            m[4:6] = False                                           # present in the file, empty
        anns[k] = gt(a["id"], 1, 1 + k % 2, m, none_at=gone[k])
    for k, r in enumerate(res):
        m = r["_masks"].copy()
        if k == 1:
            m[0:2] = False
        res[k] = det(1, 1 + (k + 1) % 2, r["score"], m, none_at={0: (7,), 2: (0, 1, 2), 4: (2, 3, 4, 5, 6, 7)}.get(k, ()))
    return {"videos": [video(1, T, H, W)], "categories": cats(2), "annotations": anns}, res, {"class_agnostic": True}


def scene_exact_fractions(seed):
    """Five pairs on rows of their own; pair k of frame t has an IoU of exactly FR[(k + t) % 5]: (gt length, track length), nested."""
    T, H, W = 5, 12, 24
    fr = [(2, 4), (1, 4), (3, 4), (1, 5), (19, 20)]                  # 1/2, 1/4, 3/4, 1/5, 19/20
    anns, res = [], []
    for k in range(5):
        g, p = np.zeros((T, H, W), bool), np.zeros((T, H, W), bool)
        for t in range(T):
            a, b = fr[(k + t) % 5]
            g[t, 2 * k + 1, 1:1 + a] = True
            p[t, 2 * k + 1, 1:1 + b] = True
        anns.append(gt(k + 1, 1, 1, g))
        res.append(det(1, 1, 0.9, p))
    return {"videos": [video(1, T, H, W)], "categories": cats(1), "annotations": anns}, res, {}


def scene_all_zero_frame(seed):
    """Frame 2: every id present, no track touches a ground truth."""
    ann, res, _ = _single(seed, 3, 3, 5)
    H, W = 24, 32
    for k, a in enumerate(ann["annotations"]):
        m = a["_masks"].copy()
        m[2] = False
        m[2, 1 + 3 * k:3 + 3 * k, 1:6] = True
        a.update(gt(a["id"], 1, 1, m))
    for k, r in enumerate(res):
        m = r["_masks"].copy()
        m[2] = False
        m[2, 14 + 3 * k:16 + 3 * k, 20:27] = True
        res[k] = det(1, 1, r["score"], m)
    return ann, res, {}


def scene_full_64x64(seed):
    """64 ground truths on an 8 x 8 grid of 8 x 12 cells, 64 tracks displaced into their neighbours' cells."""
    rng = np.random.default_rng(6400 + seed)
    T, H, W = 2, 64, 96
    anns, res = [], []
    for k in range(64):
        cy, cx = 8 * (k // 8), 12 * (k % 8)
        h, w = int(rng.integers(4, 8)), int(rng.integers(6, 12))
        anns.append(gt(k + 1, 1, 1, boxes(T, H, W, cy + int(rng.integers(0, 8 - h + 1)), cx + int(rng.integers(0, 12 - w + 1)), h, w)))
        h, w = int(rng.integers(4, 9)), int(rng.integers(6, 13))
        res.append(det(1, 1, float(rng.uniform(0.4, 0.9)), boxes(T, H, W, cy + int(rng.integers(-3, 4)), cx + int(rng.integers(-4, 5)), h, w,
                                                                  float(rng.uniform(-1, 1)), float(rng.uniform(-2, 2)))))
    order = rng.permutation(64)
    return {"videos": [video(1, T, H, W)], "categories": cats(1), "annotations": anns}, [res[i] for i in order], {}


def scene_multi_class(seed):
    """Category 2 has ground truth and no results, category 3 results and no ground truth; two videos, the second without category 1
    results."""
    rng = np.random.default_rng(500 + seed)
    H, W = 24, 32
    a1, r1 = random_tracks(rng, 1, 1, 4, H, W, 2, 3, 1)
    a2, _ = random_tracks(rng, 1, 2, 4, H, W, 2, 0, 3)
    _, r3 = random_tracks(rng, 1, 3, 4, H, W, 0, 2)
    b1, _ = random_tracks(rng, 2, 1, 3, H, W, 1, 0, 5)
    b2, r2 = random_tracks(rng, 2, 1, 3, H, W, 2, 2, 6)
    return ({"videos": [video(1, 4, H, W), video(2, 3, H, W)], "categories": cats(3), "annotations": a1 + a2 + b1 + b2}, r1 + r3 + r2, {})


def scene_no_tracks(seed):
    ann, _, _ = _single(seed, 3, 0, 4)
    return ann, [], {}


def scene_no_gt(seed):
    ann, res, _ = _single(seed, 1, 3, 4)
    ann["annotations"][0]["iscrowd"] = 1                             # the only ground truth is a crowd: dropped
    return ann, res, {}


def scene_err_size_mismatch(seed):
    ann, res, _ = _single(seed, 2, 2, 3)
    res[1] = det(1, 1, 0.5, boxes(3, 10, 10, 1, 1, 4, 4))
    return ann, res, {}, ("ValueError", "video 1: mask 3 has size [10, 10], the video is [24, 32]")


def scene_err_unknown_video(seed):
    ann, res, _ = _single(seed, 2, 2, 3)
    res[1]["video_id"] = 7
    return ann, res, {}, ("AssertionError", "Results do not correspond to current coco set")


SCENES = {"clean": scene_clean, "more_tracks_than_gt": scene_more_tracks_than_gt, "more_gt_than_tracks": scene_more_gt_than_tracks,
          "one_by_one": scene_one_by_one, "t1": scene_t1, "empty_frames": scene_empty_frames, "enter_leave": scene_enter_leave,
          "exact_fractions": scene_exact_fractions, "all_zero_frame": scene_all_zero_frame, "full_64x64": scene_full_64x64,
          "multi_class": scene_multi_class, "no_tracks": scene_no_tracks, "no_gt": scene_no_gt, "err_size_mismatch": scene_err_size_mismatch,
          "err_unknown_video": scene_err_unknown_video}


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------
def load_reference():
    """The reference's HOTA object; its scipy call is wrapped by the margin check."""
    if not hasattr(np, "float"):
        np.float = float                                             # (the one place this alias is set)
    _pkg("univs")
    _pkg("univs.evaluation", f"{REF_ROOT}/univs/evaluation")
    mod = importlib.import_module("univs.evaluation.eval_hota")
    solve = mod.linear_sum_assignment
    margins = []

    def checked(cost):
        rows, cols = solve(cost)
        total = cost[rows, cols].sum()
        for r, c in zip(rows, cols):
            if cost[r, c] < 0:                                       # a matched pair of positive score
                other = cost.copy()
                other[r, c] = 1e9
                r2, c2 = solve(other)
                margins.append(float(np.minimum(other[r2, c2], 0).sum() - total))
                if margins[-1] <= MARGIN:
                    raise Tie(f"margin {margins[-1]}")
        return rows, cols
    mod.linear_sum_assignment = checked
    return mod.HOTA(), margins


def sequence_data(gts, dts, T):
    """The `data` dictionary of one sequence from the dense masks."""
    def present(a):
        return np.array([t not in a["_none"] and bool(a["_masks"][t].any()) for t in range(T)])
    pg = np.array([present(a) for a in gts]).reshape(len(gts), T)
    pp = np.array([present(a) for a in dts]).reshape(len(dts), T)
    data = {"num_gt_ids": len(gts), "num_tracker_ids": len(dts), "num_gt_dets": int(pg.sum()), "num_tracker_dets": int(pp.sum()),
            "gt_ids": [], "tracker_ids": [], "similarity_scores": []}
    for t in range(T):
        gi, pi = np.flatnonzero(pg[:, t]), np.flatnonzero(pp[:, t])
        sim = np.zeros((len(gi), len(pi)), np.float64)
        for i, g in enumerate(gi):
            for j, p in enumerate(pi):
                mg, mp = gts[g]["_masks"][t], dts[p]["_masks"][t]
                inter = np.int64((mg & mp).sum())
                sim[i, j] = np.float64(inter) / np.float64(np.int64(mg.sum()) + np.int64(mp.sum()) - inter)
        data["gt_ids"].append(gi)
        data["tracker_ids"].append(pi)
        data["similarity_scores"].append(sim)
    return data


def run_reference(metric, ann, res, score_thresh=0.0, class_agnostic=False):
    """-> (sequences {(video, class): res}, per class, class-averaged, detection-averaged), sequences in the file's video order."""
    keys = ["all"] if class_agnostic else sorted(c["id"] for c in ann["categories"])
    seqs = {}
    for v in ann["videos"]:
        gts = [a for a in ann["annotations"] if a["video_id"] == v["id"] and not a["iscrowd"]]
        dts = [d for d in res if d["video_id"] == v["id"] and d["score"] >= score_thresh]
        for key in keys:
            g = [a for a in gts if class_agnostic or a["category_id"] == key]
            d = [a for a in dts if class_agnostic or a["category_id"] == key]
            if g or d:
                seqs[v["id"], key] = metric.eval_sequence(sequence_data(g, d, v["length"]))
    per_class = {}
    for key in keys:
        mine = {vid: r for (vid, k), r in seqs.items() if k == key}
        if mine:
            per_class[key] = metric.combine_sequences(mine)
    return seqs, per_class, metric.combine_classes_class_averaged(per_class), metric.combine_classes_det_averaged(per_class)


def strip(records):
    return [{k: v for k, v in r.items() if not k.startswith("_")} for r in records]


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    metric, margins = load_reference()
    fields = metric.fields
    for name, make in SCENES.items():
        for seed in range(50):
            ann, res, opts, *error = make(seed)
            del margins[:]
            try:
                out = None if error else run_reference(metric, ann, res, **opts)
                break
            except Tie as e:
                print(f"{name}: seed {seed}: {e}; next seed")
        else:
            raise SystemExit(f"{name}: no seed without a tie")
        rec = {"gt_json": np.array(json.dumps(dict(ann, annotations=strip(ann["annotations"])))), "results_json": np.array(json.dumps(strip(res))),
               "score_thresh": np.float64(opts.get("score_thresh", 0.0)), "class_agnostic": np.bool_(opts.get("class_agnostic", False))}
        if error:
            rec["error"], rec["error_text"] = np.array(error[0][0]), np.array(error[0][1])
        else:
            seqs, per_class, cls_av, det_av = out
            rec["seq_keys"] = np.array([f"{vid}__{key}" for vid, key in seqs])
            rec["cls_keys"] = np.array([str(k) for k in per_class])
            for (vid, key), r in seqs.items():
                for f in fields:
                    rec[f"seq__{vid}__{key}__{f}"] = np.asarray(r[f], np.float64)
            for key, r in per_class.items():
                for f in fields:
                    rec[f"cls__{key}__{f}"] = np.asarray(r[f], np.float64)
            for f in fields:
                rec[f"cls_av__{f}"] = np.asarray(cls_av[f], np.float64)
                rec[f"det_av__{f}"] = np.asarray(det_av[f], np.float64)
            rec["min_margin"] = np.float64(min(margins) if margins else np.inf)
        path = os.path.join(GOLDEN, f"g34_hota_{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) <= 262144, f"{name}: {os.path.getsize(path)} bytes"
        hota = "" if error else f"HOTA {100 * np.mean(out[3]['HOTA']):.3f} frames solved {len(margins)} min margin {rec['min_margin']:.3g}"
        print(name, f"seed {seed}", os.path.getsize(path), "bytes", rec.get("error", ""), hota)


if __name__ == "__main__":
    main()
