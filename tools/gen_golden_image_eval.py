"""Golden fixtures of the per-image panoptic scoring (tests/golden/g38_image_eval_*.npz): the reference's own
`vpq_compute_single_core(categories, nframes=1, ...)` and `PQStat.pq_average` (univs/evaluation/eval_vpq_vps.py:24-234) run on small
synthetic COCO-panoptic trees in a temporary directory, every image a tube of one frame -- panopticapi's `pq_compute_single_core`.

The script is imported by path (it needs numpy, PIL and tqdm only).  Each image is scored by one call, its `PQStat` added to the
total (`vpq_stat += tmp`, as the reference's `vpq_compute` does per video), then `pq_average` for all, things and stuff.

Each fixture holds the PNG pixels as id maps (id = R + 256 G + 65536 B; the test paints the PNGs), the ground truth and the
predictions as json strings and, for a scene the reference scores: the per-category iou / tp / fp / fn and the All / Things / Stuff
averages (nan where a group has no class: the reference divides by zero there, recorded as nan).  An error scene holds the
exception's type name and text instead.

Scenes: `clean` (three images, things and stuff, all matched); `half` (an IoU of exactly 0.5: no match); `void` (a prediction more
than half on VOID: ignored); `crowd` (a prediction mostly on a crowd of its class: ignored; the crowd is no false negative);
`pred_only` (a class present only in the prediction); `two_of_a_class` (two segments of one class, one matched); and the three
KeyError scenes `err_png_not_json`, `err_unknown_category`, `err_json_not_png`.

    python tools/gen_golden_image_eval.py     # needs the reference tree (dev container only)
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
from oracle.ref_harness import REF_ROOT                 # noqa: E402  (UNIVS_REFERENCE_ROOT)

REF_EVAL = os.path.join(REF_ROOT, "univs", "evaluation")
H, W = 40, 60
CATEGORIES = [{"id": 7, "name": "person", "isthing": 1}, {"id": 9, "name": "car", "isthing": 1}, {"id": 30, "name": "sky", "isthing": 0},
              {"id": 41, "name": "road", "isthing": 0}]


def paint(segs):
    """segs: [(id, category, iscrowd, (y0, y1, x0, x1))] painted in order -> (ids int32 [H, W], segments_info from the pixels)."""
    pan = np.zeros((H, W), dtype=np.int32)
    for sid, _, _, (y0, y1, x0, x1) in segs:
        pan[y0:y1, x0:x1] = sid
    info = []
    for sid, cat, crowd, _ in segs:
        area = int((pan == sid).sum())
        if area:
            info.append({"id": int(sid), "category_id": int(cat), "iscrowd": int(crowd), "area": area})
    return pan, info


def image(name, gt_segs, pred_segs):
    gt, gt_info = paint(gt_segs)
    pred, pred_info = paint(pred_segs)
    for el in pred_info:                                             # a prediction's record carries no crowd flag and no area
        del el["iscrowd"], el["area"]
    return {"image_id": name, "gt": gt, "pred": pred, "gt_info": gt_info, "pred_info": pred_info}


def scene_clean():
    return [image("a", [(300, 30, 0, (0, 20, 0, W)), (70000, 41, 0, (20, H, 0, W)), (5, 7, 0, (10, 30, 5, 20)), (6, 9, 0, (25, 38, 30, 55))],
                  [(1, 30, 0, (0, 21, 0, W)), (2, 41, 0, (21, H, 0, W)), (3, 7, 0, (10, 30, 5, 21)), (4, 9, 0, (25, 38, 31, 55))]),
            image("b", [(11, 30, 0, (0, 15, 0, W)), (12, 41, 0, (15, H, 0, W)), (13, 7, 0, (5, 25, 40, 50))],
                  [(1, 30, 0, (0, 15, 0, W)), (2, 41, 0, (15, H, 0, W)), (3, 7, 0, (6, 25, 40, 50))]),
            image("c", [(21, 41, 0, (0, H, 0, W)), (22, 9, 0, (10, 20, 10, 30)), (23, 9, 0, (25, 35, 35, 55))],
                  [(1, 41, 0, (0, H, 0, W)), (2, 9, 0, (10, 20, 10, 29)), (3, 9, 0, (25, 35, 36, 55))])]


def scene_half():
    # the person's ground truth is 10 x 20 = 200 pixels, the prediction its left half (100): IoU = 100 / 200 = 0.5 exactly, no match
    return [image("a", [(1, 41, 0, (0, H, 0, W)), (2, 7, 0, (10, 20, 10, 30))], [(1, 41, 0, (0, H, 0, W)), (2, 7, 0, (10, 20, 10, 20))])]


def scene_void():
    # rows 20.. are VOID in the ground truth; the predicted car lies 8 of its 10 rows there: ignored, not a false positive
    return [image("a", [(1, 30, 0, (0, 20, 0, W))], [(1, 30, 0, (0, 20, 0, W)), (2, 9, 0, (18, 28, 10, 30))])]


def scene_crowd():
    # a crowd of persons; one predicted person mostly on it (ignored), one half on it and half elsewhere (a false positive)
    return [image("a", [(1, 41, 0, (0, H, 0, W)), (2, 7, 1, (5, 25, 5, 35)), (3, 7, 0, (28, 38, 40, 55))],
                  [(1, 41, 0, (0, H, 0, W)), (2, 7, 0, (8, 22, 8, 30)), (3, 7, 0, (28, 38, 41, 55)), (4, 7, 0, (10, 20, 30, 40))])]


def scene_pred_only():
    return [image("a", [(1, 30, 0, (0, 20, 0, W)), (2, 41, 0, (20, H, 0, W))],
                  [(1, 30, 0, (0, 20, 0, W)), (2, 41, 0, (20, H, 0, W)), (3, 9, 0, (22, 30, 10, 30))])]


def scene_two_of_a_class():
    return [image("a", [(1, 41, 0, (0, H, 0, W)), (2, 7, 0, (5, 15, 5, 25)), (3, 7, 0, (20, 35, 30, 50))],
                  [(1, 41, 0, (0, H, 0, W)), (2, 7, 0, (5, 15, 6, 25)), (3, 7, 0, (20, 35, 42, 58))])]


def scene_err_png_not_json():
    ims = scene_two_of_a_class()
    ims[0]["pred_info"] = ims[0]["pred_info"][:-1]
    return ims


def scene_err_unknown_category():
    ims = scene_two_of_a_class()
    ims[0]["pred_info"][1]["category_id"] = 99
    return ims


def scene_err_json_not_png():
    ims = scene_two_of_a_class()
    ims[0]["pred_info"].append({"id": 77, "category_id": 7})
    return ims


SCENES = {"clean": scene_clean, "half": scene_half, "void": scene_void, "crowd": scene_crowd, "pred_only": scene_pred_only,
          "two_of_a_class": scene_two_of_a_class, "err_png_not_json": scene_err_png_not_json,
          "err_unknown_category": scene_err_unknown_category, "err_json_not_png": scene_err_json_not_png}


def ids_to_rgb(ids):
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


def jsons_of(images):
    gt = {"categories": CATEGORIES, "images": [{"id": im["image_id"], "file_name": im["image_id"] + ".jpg"} for im in images],
          "annotations": [{"image_id": im["image_id"], "file_name": im["image_id"] + ".png", "segments_info": im["gt_info"]} for im in images]}
    pred = {"annotations": [{"image_id": im["image_id"], "file_name": im["image_id"] + ".png", "segments_info": im["pred_info"]} for im in images]}
    return gt, pred


def load_reference():
    sys.path.insert(0, REF_EVAL)
    spec = importlib.util.spec_from_file_location("eval_vpq_vps", os.path.join(REF_EVAL, "eval_vpq_vps.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["eval_vpq_vps"] = mod
    spec.loader.exec_module(mod)
    return mod


def run_reference(ref, root, images, gt_json, pred_json):
    categories = {el["id"]: el for el in gt_json["categories"]}
    total = ref.PQStat()
    for im, g, p in zip(images, gt_json["annotations"], pred_json["annotations"]):
        paths = []
        for side in ("gt", "pred"):
            paths.append(os.path.join(root, side + "_" + im["image_id"] + ".png"))
            Image.fromarray(ids_to_rgb(im[side])).save(paths[-1])
        total += ref.vpq_compute_single_core(categories, 1, [(g, p, paths[0], paths[1], None)])
    out = []
    for isthing in (None, True, False):
        try:
            out.append(total.pq_average(categories, isthing))
        except ZeroDivisionError:
            out.append(({"pq": np.nan, "sq": np.nan, "rq": np.nan, "n": 0}, None))
    return out


def main():
    ref = load_reference()
    os.makedirs(GOLDEN, exist_ok=True)
    for name, make in SCENES.items():
        images = make()
        gt_json, pred_json = jsons_of(images)
        rec = {"image_ids": np.array([im["image_id"] for im in images]), "gt_json": np.array(json.dumps(gt_json)),
               "pred_json": np.array(json.dumps(pred_json))}
        for im in images:
            rec["gt_" + im["image_id"]] = im["gt"]
            rec["pred_" + im["image_id"]] = im["pred"]
        with tempfile.TemporaryDirectory() as root:
            if name.startswith("err_"):
                try:
                    run_reference(ref, root, images, gt_json, pred_json)
                except KeyError as e:
                    rec["error"], rec["error_text"] = np.array(type(e).__name__), np.array(e.args[0])
                assert "error" in rec, f"{name}: the reference did not raise"
            else:
                (all_avg, per_class), (th_avg, _), (st_avg, _) = run_reference(ref, root, images, gt_json, pred_json)
                cats = list(per_class)
                rec["cats"] = np.array(cats, dtype=np.int64)
                rec["iou"] = np.array([per_class[c]["iou"] for c in cats], dtype=np.float64)
                for k in ("tp", "fp", "fn"):
                    rec[k] = np.array([per_class[c][k] for c in cats], dtype=np.int64)
                rec["avg"] = np.array([[a["pq"], a["sq"], a["rq"], a["n"]] for a in (all_avg, th_avg, st_avg)], dtype=np.float64)
                print(name, {c: (per_class[c]["tp"], per_class[c]["fp"], per_class[c]["fn"], round(per_class[c]["iou"], 4)) for c in cats})
        path = os.path.join(GOLDEN, f"g38_image_eval_{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, os.path.getsize(path), "bytes", rec.get("error_text", ""))


if __name__ == "__main__":
    main()
