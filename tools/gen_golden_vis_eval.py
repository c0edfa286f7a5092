"""Golden fixtures of the YouTube-VIS scoring (tests/golden/g29_vis_eval_*.npz): the reference's own `YTVOS` (createIndex, loadRes),
`YTVOSeval` (evaluate, accumulate, summarize) and `YTVISEvaluator._derive_coco_results`, run unmodified on small synthetic annotation
and result sets (univs/data/datasets/ytvis_api/ytvos.py, ytvoseval.py; univs/evaluation/ytvis_evaluation.py).

The evaluator object is made without its constructor (which needs detectron2's MetadataCatalog).  Stand-ins: detectron2's inert bases
from `oracle.ref_harness.ref_evaluators()`, `create_small_table` (its text is only logged), and `pycocotools.mask`, which is absent
here: `area`, `merge` (with and without `intersect`), `frPyObjects` for uncompressed RLE, `toBbox`, `encode` and `decode`, built on
decoded numpy masks and this repository's own string coder (univs_amd/inference/results.py) -- so the fixtures pin everything the
reference does EXCEPT pycocotools' own code.

Each fixture holds the annotation and result JSON as strings (`gt_json`, `results_json`), the class names, and for a scene the
reference's `stats` [12], `precision`, `recall`, `scores`, the keys (`ious_keys` [n, 2]) and blocks (`ious_<i>`) of every ious entry of
non-zero length, the derived dictionary (`derived_keys`, `derived_values`) and the twelve lines `summarize` prints (`lines`).  An error
scene holds the exception's type name.

Scenes: `clean` (3 videos, 3 categories); `score_ties` (equal scores within and across videos); `crowd` (an iscrowd ground truth
matched by two detections); `none_frames` (None on both sides, a detection present only where the ground truth is absent);
`over_maxdets` (103 detections in one (video, category) on 12 x 16 frames); `area_ranges` (300 x 400 frames, avg_area on both sides of
128^2 and 256^2, unmatched detections outside a range); `absent_category` (a category without ground truth, one with ground truth and
no detections); `mixed_gt_rle` (compressed and uncompressed ground-truth codes); `zero_union` (a detection / ground-truth pair that is
empty everywhere); and the error scenes `err_unknown_video`, `err_not_a_list`.

    python tools/gen_golden_vis_eval.py     # needs the reference tree (dev container only)
"""
import contextlib
import copy
import importlib
import io
import json
import logging
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
from oracle.ref_harness import REF_ROOT, _pkg, ref_evaluators  # noqa: E402  (UNIVS_REFERENCE_ROOT)
from univs_amd.inference.results import rle_decode, rle_encode_masks  # noqa: E402


# ------------------------------------------------------------------------------------------------------------------------------------
# synthetic annotation and result sets
# ------------------------------------------------------------------------------------------------------------------------------------
def ell(T, H, W, cy, cx, ry, rx, vy=0.0, vx=0.0, wob=0.0):
    """bool [T, H, W]: an ellipse moving by (vy, vx) per frame and breathing by `wob` pixels."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((T, H, W), bool)
    for t in range(T):
        a, b = max(ry + wob * np.sin(0.9 * t), 0.5), max(rx + wob * np.cos(0.7 * t), 0.5)
        out[t] = ((yy - cy - vy * t) / a) ** 2 + ((xx - cx - vx * t) / b) ** 2 <= 1.0
    return out


def enc(masks, none_at=(), uncompressed=False):
    """One RLE per frame (None at the frames `none_at`), and the areas YouTube-VIS annotations carry beside them."""
    rles = rle_encode_masks(torch.from_numpy(masks))
    if uncompressed:
        from univs_amd.inference.results import rle_counts
        rles = [{"size": r["size"], "counts": [int(c) for c in rle_counts(r)]} for r in rles]
    segs = [None if t in none_at else r for t, r in enumerate(rles)]
    areas = [None if t in none_at else int(m.sum()) for t, m in enumerate(masks)]
    return segs, areas


def video(vid, T, H, W):
    return {"id": vid, "height": H, "width": W, "length": T, "file_names": ["v%d/%05d.jpg" % (vid, t) for t in range(T)]}


def gt(aid, vid, cat, masks, iscrowd=0, none_at=(), uncompressed=False):
    segs, areas = enc(masks, none_at, uncompressed)
    return {"id": aid, "video_id": vid, "category_id": cat, "iscrowd": iscrowd, "segmentations": segs, "areas": areas}


def det(vid, cat, score, masks, none_at=()):
    segs, _ = enc(masks, none_at)
    return {"video_id": vid, "score": score, "category_id": cat, "segmentations": segs, "height": masks.shape[1], "width": masks.shape[2]}


def cats(n):
    return [{"id": k + 1, "name": ("person", "dog", "car", "bird")[k]} for k in range(n)]


def scene_clean():
    H, W = 24, 32
    shapes = {1: [(1, 8, 9, 5, 6, 0.5, 1.0, 0.5), (2, 16, 22, 4, 5, -0.5, 0.5, 0.8), (1, 18, 6, 3, 4, 0, 0.5, 0.3)],
              2: [(2, 10, 12, 6, 7, 0.3, 0.8, 1.0), (3, 15, 25, 4, 4, 0, -1.0, 0.5)],
              3: [(3, 12, 16, 7, 9, 0, 0, 1.0), (1, 5, 5, 3, 3, 1.0, 1.0, 0), (2, 19, 26, 3, 4, 0, -0.5, 0.2)]}
    frames = {1: 4, 2: 5, 3: 3}
    rng = np.random.default_rng(1)
    anns, res, aid = [], [], 1
    for vid, objs in shapes.items():
        T = frames[vid]
        for (c, cy, cx, ry, rx, vy, vx, wob) in objs:
            anns.append(gt(aid, vid, c, ell(T, H, W, cy, cx, ry, rx, vy, vx, wob)))
            aid += 1
            j = rng.uniform(-1.5, 1.5, 4)
            res.append(det(vid, c, float(rng.uniform(0.3, 0.95)), ell(T, H, W, cy + j[0], cx + j[1], ry + j[2] / 2, rx + j[3] / 2, vy, vx, wob)))
        res.append(det(vid, int(rng.integers(1, 4)), float(rng.uniform(0.05, 0.5)), ell(T, H, W, 20, 28, 2, 3)))            # a false positive
        c, cy, cx, ry, rx, vy, vx, wob = objs[0]
        res.append(det(vid, c, float(rng.uniform(0.2, 0.6)), ell(T, H, W, cy + 3, cx - 2, ry, rx, vy, vx, wob)))            # a duplicate
    return {"videos": [video(v, frames[v], H, W) for v in shapes], "categories": cats(3), "annotations": anns}, res


def scene_score_ties():
    H, W, T = 20, 28, 3
    anns = [gt(1, 1, 1, ell(T, H, W, 7, 8, 4, 5)), gt(2, 1, 1, ell(T, H, W, 13, 20, 4, 5)), gt(3, 2, 1, ell(T, H, W, 10, 14, 5, 6)),
            gt(4, 2, 2, ell(T, H, W, 5, 5, 3, 3))]
    res = [det(1, 1, 0.5, ell(T, H, W, 8, 9, 4, 5)), det(1, 1, 0.5, ell(T, H, W, 13, 19, 4, 5)), det(1, 1, 0.5, ell(T, H, W, 7, 8, 4, 4)),
           det(2, 1, 0.5, ell(T, H, W, 10, 15, 5, 6)), det(2, 1, 0.7, ell(T, H, W, 15, 5, 2, 2)), det(2, 2, 0.5, ell(T, H, W, 5, 6, 3, 3)),
           det(1, 1, 0.7, ell(T, H, W, 2, 25, 2, 2)), det(2, 2, 0.5, ell(T, H, W, 15, 22, 3, 3))]
    return {"videos": [video(1, T, H, W), video(2, T, H, W)], "categories": cats(2), "annotations": anns}, res


def scene_crowd():
    H, W, T = 24, 32, 3
    anns = [gt(1, 1, 1, ell(T, H, W, 12, 10, 8, 8), iscrowd=1), gt(2, 1, 1, ell(T, H, W, 12, 25, 4, 4))]
    big = ell(T, H, W, 12, 10, 8, 8)
    res = [det(1, 1, 0.9, big & ell(T, H, W, 12, 9, 8, 7)), det(1, 1, 0.8, ell(T, H, W, 12, 11, 7, 8)), det(1, 1, 0.7, ell(T, H, W, 12, 25, 4, 4)),
           det(1, 1, 0.6, ell(T, H, W, 13, 24, 4, 4))]
    return {"videos": [video(1, T, H, W)], "categories": cats(1), "annotations": anns}, res


def scene_none_frames():
    H, W, T = 20, 28, 6
    a = ell(T, H, W, 8, 8, 4, 5, 0.5, 1.0)
    b = ell(T, H, W, 14, 20, 4, 4, 0, -0.5)
    anns = [gt(1, 1, 1, a, none_at=(0, 1)), gt(2, 1, 2, b, none_at=(4, 5))]
    res = [det(1, 1, 0.9, ell(T, H, W, 8, 9, 4, 5, 0.5, 1.0), none_at=(1, 5)), det(1, 2, 0.8, b, none_at=(0, 1, 2, 3)),
           det(1, 1, 0.4, a, none_at=(2, 3, 4, 5)), det(1, 2, 0.3, ell(T, H, W, 14, 19, 4, 4, 0, -0.5))]
    return {"videos": [video(1, T, H, W)], "categories": cats(2), "annotations": anns}, res


def scene_over_maxdets():
    H, W, T = 12, 16, 2
    anns = [gt(1, 1, 1, ell(T, H, W, 4, 5, 3, 3)), gt(2, 1, 1, ell(T, H, W, 8, 12, 2, 3))]
    rng = np.random.default_rng(3)
    res = []
    for k in range(103):
        cy, cx = (4, 5) if k % 2 == 0 else (8, 12)
        res.append(det(1, 1, float(rng.uniform(0.01, 0.99)), ell(T, H, W, cy + rng.uniform(-3, 3), cx + rng.uniform(-3, 3), 3, 3)))
    res[101]["score"], res[102]["score"] = 0.995, 0.001                   # the best one arrives after the first hundred
    res[101]["segmentations"] = res[0]["segmentations"][:]
    return {"videos": [video(1, T, H, W)], "categories": cats(1), "annotations": anns}, res


def scene_area_ranges():
    H, W, T = 300, 400, 2
    objs = [(1, 40, 50, 20, 20), (1, 150, 120, 100, 100), (1, 150, 200, 146, 180), (1, 260, 360, 30, 35), (2, 100, 300, 72, 72),
            (2, 150, 200, 140, 150)]                                        # avg_area near 1 257, 31 416, 82 561, 3 299, 16 286, 65 973
    anns = [gt(i + 1, 1, c, ell(T, H, W, cy, cx, ry, rx, 1, 2, 1.5)) for i, (c, cy, cx, ry, rx) in enumerate(objs)]
    rng = np.random.default_rng(4)
    res = [det(1, c, float(rng.uniform(0.4, 0.95)), ell(T, H, W, cy + 2, cx - 3, ry + 1, rx - 1, 1, 2, 1.5)) for (c, cy, cx, ry, rx) in objs]
    res += [det(1, 1, 0.35, ell(T, H, W, 250, 60, 25, 25)), det(1, 1, 0.3, ell(T, H, W, 200, 200, 90, 95)), det(1, 2, 0.25, ell(T, H, W, 150, 200, 149, 190)),
            det(1, 2, 0.2, ell(T, H, W, 280, 20, 10, 12))]                  # unmatched, small / medium / large / small
    return {"videos": [video(1, T, H, W)], "categories": cats(2), "annotations": anns}, res


def scene_absent_category():
    H, W, T = 20, 28, 3
    anns = [gt(1, 1, 1, ell(T, H, W, 7, 8, 4, 5)), gt(2, 1, 2, ell(T, H, W, 13, 20, 4, 5)), gt(3, 2, 2, ell(T, H, W, 10, 14, 5, 6))]
    res = [det(1, 1, 0.9, ell(T, H, W, 7, 9, 4, 5)), det(1, 3, 0.8, ell(T, H, W, 13, 20, 4, 5)), det(2, 3, 0.7, ell(T, H, W, 10, 14, 5, 6)),
           det(2, 1, 0.6, ell(T, H, W, 4, 4, 2, 2))]
    return {"videos": [video(1, T, H, W), video(2, T, H, W)], "categories": cats(3), "annotations": anns}, res


def scene_mixed_gt_rle():
    H, W, T = 22, 30, 4
    anns = [gt(1, 1, 1, ell(T, H, W, 7, 8, 4, 5, 0.5, 0.5), uncompressed=True), gt(2, 1, 1, ell(T, H, W, 14, 20, 5, 6, 0, -1)),
            gt(3, 1, 2, ell(T, H, W, 16, 6, 3, 4), uncompressed=True, none_at=(3,))]
    anns[1]["segmentations"][2] = enc(ell(T, H, W, 14, 20, 5, 6, 0, -1), uncompressed=True)[0][2]      # both kinds inside one annotation
    full = np.zeros((T, H, W), bool)
    full[:, 0, 0] = True                                                  # a leading foreground pixel: the code opens with an empty run
    full[:, -1, -1] = True
    anns.append(gt(4, 1, 2, full, uncompressed=True))
    res = [det(1, 1, 0.9, ell(T, H, W, 7, 9, 4, 5, 0.5, 0.5)), det(1, 1, 0.8, ell(T, H, W, 14, 19, 5, 6, 0, -1)), det(1, 2, 0.7, ell(T, H, W, 16, 6, 3, 3)),
           det(1, 2, 0.6, full)]
    return {"videos": [video(1, T, H, W)], "categories": cats(2), "annotations": anns}, res


def scene_zero_union():
    H, W, T = 16, 20, 3
    empty = np.zeros((T, H, W), bool)
    anns = [gt(1, 1, 1, empty, none_at=(0, 1, 2)), gt(2, 1, 1, ell(T, H, W, 8, 10, 4, 5))]
    res = [det(1, 1, 0.9, empty), det(1, 1, 0.8, ell(T, H, W, 8, 11, 4, 5)), det(1, 1, 0.7, empty, none_at=(0, 1, 2))]
    return {"videos": [video(1, T, H, W)], "categories": cats(1), "annotations": anns}, res


def scene_err_unknown_video():
    ann, res = scene_crowd()
    res[1]["video_id"] = 7
    return ann, res, AssertionError


def scene_err_not_a_list():
    ann, res = scene_crowd()
    return ann, {"results": res}, AssertionError


SCENES = {"clean": scene_clean, "score_ties": scene_score_ties, "crowd": scene_crowd, "none_frames": scene_none_frames,
          "over_maxdets": scene_over_maxdets, "area_ranges": scene_area_ranges, "absent_category": scene_absent_category,
          "mixed_gt_rle": scene_mixed_gt_rle, "zero_union": scene_zero_union, "err_unknown_video": scene_err_unknown_video,
          "err_not_a_list": scene_err_not_a_list}


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------
def mask_stand_in():
    """`pycocotools.mask` on decoded numpy masks and the repository's string coder (what its documentation states of each call)."""
    m = types.ModuleType("pycocotools.mask")

    def _dec(rle):
        c = rle["counts"]
        return rle_decode({"size": rle["size"], "counts": c.decode("ascii") if isinstance(c, bytes) else c})

    def _enc(mask):
        r = rle_encode_masks(torch.from_numpy(np.ascontiguousarray(mask).astype(bool)))[0]
        return {"size": r["size"], "counts": r["counts"].encode("ascii")}

    def area(rles):
        return np.uint32(_dec(rles).sum()) if isinstance(rles, dict) else np.array([_dec(r).sum() for r in rles], dtype=np.uint32)

    def merge(rles, intersect=False):
        stack = np.stack([_dec(r) for r in rles]).astype(bool)
        return _enc(stack.all(0) if intersect else stack.any(0))

    def fr_py_objects(obj, h, w):
        def one(o):
            if not (isinstance(o, dict) and isinstance(o["counts"], list)):
                raise NotImplementedError("only uncompressed RLE")
            flat = np.repeat(np.arange(len(o["counts"])) % 2, o["counts"]).astype(np.uint8)
            assert flat.shape[0] == h * w and list(o["size"]) == [h, w]
            return _enc(flat.reshape(w, h).T)
        return [one(o) for o in obj] if isinstance(obj, list) else one(obj)

    def to_bbox(rle):
        ys, xs = np.nonzero(_dec(rle))
        if len(ys) == 0:
            return np.zeros(4)
        return np.array([xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1], dtype=np.float64)

    def encode(arr):
        return [_enc(arr[:, :, i]) for i in range(arr.shape[2])] if arr.ndim == 3 else _enc(arr)

    def decode(rle):
        return _dec(rle) if isinstance(rle, dict) else np.stack([_dec(r) for r in rle], axis=2)
    m.area, m.merge, m.frPyObjects, m.toBbox, m.encode, m.decode = area, merge, fr_py_objects, to_bbox, encode, decode
    return m


def load_reference():
    """(YTVOS, YTVOSeval, YTVISEvaluator) of the reference, imported from its files with the stand-ins of the module docstring."""
    ref_evaluators()                                                 # detectron2's inert bases, the `univs` parent package
    pc = _pkg("pycocotools")
    pc.mask = mask_stand_in()
    sys.modules["pycocotools.mask"] = pc.mask
    sys.modules["detectron2.evaluation"].COCOEvaluator = type("COCOEvaluator", (), {})
    lg = _pkg("detectron2.utils.logger")
    lg.create_small_table = lambda d: " | ".join(f"{k}: {v:.3f}" for k, v in d.items())
    _pkg("univs.data")
    _pkg("univs.data.datasets")
    _pkg("univs.data.datasets.ytvis_api", f"{REF_ROOT}/univs/data/datasets/ytvis_api")
    _pkg("univs.evaluation", f"{REF_ROOT}/univs/evaluation")
    import matplotlib
    matplotlib.use("Agg")
    ytvos = importlib.import_module("univs.data.datasets.ytvis_api.ytvos")
    ytvoseval = importlib.import_module("univs.data.datasets.ytvis_api.ytvoseval")
    ev = importlib.import_module("univs.evaluation.ytvis_evaluation")
    return ytvos.YTVOS, ytvoseval.YTVOSeval, ev.YTVISEvaluator


def run_reference(ref, ann, res, names):
    YTVOS, YTVOSeval, YTVISEvaluator = ref
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        api = YTVOS()
        api.dataset = copy.deepcopy(ann)
        api.createIndex()
        e = YTVOSeval(api, api.loadRes(copy.deepcopy(res)), iouType="segm")
        e.evaluate()
        e.accumulate()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        e.summarize()
    with contextlib.redirect_stdout(sink):
        shell = object.__new__(YTVISEvaluator)
        shell._logger = logging.getLogger("gen_golden_vis_eval")
        derived = shell._derive_coco_results(e, "segm", class_names=names)
    return e, out.getvalue().splitlines(), derived


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    ref = load_reference()
    for name, make in SCENES.items():
        ann, res, *error = make()
        names = [c["name"] for c in ann["categories"]]
        rec = {"gt_json": np.array(json.dumps(ann)), "results_json": np.array(json.dumps(res)), "class_names": np.array(names)}
        if error:
            try:
                run_reference(ref, ann, res, names)
            except error[0] as e:
                rec["error"] = np.array(type(e).__name__)
            assert "error" in rec, f"{name}: the reference did not raise"
        else:
            e, lines, derived = run_reference(ref, ann, res, names)
            assert len(lines) == 12
            rec["stats"] = np.asarray(e.stats, np.float64)
            for k in ("precision", "recall", "scores"):
                rec[k] = np.asarray(e.eval[k], np.float64)
            keys = [k for k, v in e.ious.items() if len(v) > 0]
            rec["ious_keys"] = np.asarray(keys, np.int64).reshape(-1, 2)
            for i, k in enumerate(keys):
                rec[f"ious_{i}"] = np.asarray(e.ious[k], np.float64)
            rec["derived_keys"] = np.array(list(derived.keys()))
            rec["derived_values"] = np.array(list(derived.values()), np.float64)
            rec["lines"] = np.array(lines)
        path = os.path.join(GOLDEN, f"g29_vis_eval_{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) <= 262144, f"{name}: {os.path.getsize(path)} bytes"
        print(name, os.path.getsize(path), "bytes", rec.get("error", ""), *rec.get("lines", []), sep="\n  ")


if __name__ == "__main__":
    main()
