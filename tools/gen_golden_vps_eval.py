"""Golden fixtures of the VPS scoring (tests/golden/g26_vps_eval_*.npz): the reference's own `eval_vpq_vps.main` and
`eval_stq_vps.main` (univs/evaluation/) run on small synthetic VIPSeg trees in a temporary directory.

The two scripts are imported by path (they need numpy, PIL and tqdm only); `np.bool` is restored first, `STQuality` uses the removed
alias.  `PQStat.pq_average` and `STQuality.result` are wrapped to keep what they return; nothing else of the reference runs differently.

Each fixture holds the PNG pixels as id maps (id = R + 256 G + 65536 B; the test paints the PNGs), both JSONs as strings and, for a
scene the reference scores: per window length the per-category iou / tp / fp / fn and the All / Things / Stuff averages, the text of
every result file, and STQ / AQ / IoU with the per-sequence lists.  An error scene holds the exception's type name instead.

Scenes: `clean` (3 videos of 9, 10 and 12 frames, things and stuff, hits / misses / false alarms in both); `crowd_void` (a crowd
segment, VOID regions, predictions mostly on the crowd region and mostly on VOID: both ignored); `enter_leave` (a thing enters late,
another leaves, an id with pixels that one frame's record does not list); `short` (a 5-frame video: no window of 6 or 8); `big_tables`
(241 x 241 ids: beyond the kernel's LDS bound); and one error scene per KeyError / assertion path of the VPQ script.

    python tools/gen_golden_vps_eval.py     # needs the reference tree (dev container only)
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
H, W = 96, 160

CATEGORIES = [{"id": 0, "name": "sky", "isthing": 0, "color": [70, 130, 180]}, {"id": 1, "name": "road", "isthing": 0, "color": [128, 64, 128]},
              {"id": 2, "name": "wall", "isthing": 0, "color": [102, 102, 156]}, {"id": 3, "name": "person", "isthing": 1, "color": [220, 20, 60]},
              {"id": 4, "name": "car", "isthing": 1, "color": [0, 0, 142]}, {"id": 5, "name": "dog", "isthing": 1, "color": [0, 80, 100]}]


def seg_id(k):
    """Distinct ids with all three bytes non-zero."""
    return (k * 37 + 11) % 255 + 1 + 256 * ((k * 5 + 3) % 255 + 1) + 65536 * (k % 200 + 1)


def rect(y0, y1, x0, x1, dy=0, dx=0, first=0, last=10 ** 6):
    """A rectangle that moves (dy, dx) per frame and exists in frames [first, last]."""
    def at(t):
        if not first <= t <= last:
            return None
        return (max(0, y0 + dy * t), min(H, y1 + dy * t), max(0, x0 + dx * t), min(W, x1 + dx * t))
    return at


def paint(T, segs, size=(H, W)):
    """segs: [(id, category, iscrowd, rect)] painted in order -> (ids int32 [T, h, w], per-frame segments_info from the pixels)."""
    pan = np.zeros((T,) + size, dtype=np.int32)
    for t in range(T):
        for sid, _, _, at in segs:
            r = at(t)
            if r is not None and r[0] < r[1] and r[2] < r[3]:
                pan[t, r[0]:r[1], r[2]:r[3]] = sid
    frames = []
    for t in range(T):
        info = []
        for sid, cat, crowd, _ in segs:
            area = int((pan[t] == sid).sum())
            if area:
                info.append({"id": int(sid), "category_id": int(cat), "iscrowd": int(crowd), "area": area})
        frames.append(info)
    return pan, frames


def video(vid, T, gt_segs, pred_segs, pred_size=(H, W)):
    gt, gt_info = paint(T, gt_segs)
    pred, pred_info = paint(T, pred_segs, pred_size)
    names = ["%08d.png" % (t + 1) for t in range(T)]
    return {"video_id": vid, "names": names, "gt": gt, "pred": pred, "gt_info": gt_info, "pred_info": pred_info}


def street(vid, T, shift=0):
    """Things and stuff with a hit, a miss and a false alarm in both."""
    S = [seg_id(k + shift) for k in range(12)]
    gt = [(S[0], 0, 0, rect(0, 32, 0, W)), (S[1], 1, 0, rect(32, 64, 0, W)), (S[2], 2, 0, rect(64, 96, 0, W)),
          (S[3], 3, 0, rect(20, 50, 10, 30, dx=3)), (S[4], 4, 0, rect(60, 85, 100, 150, dx=-2)), (S[5], 5, 0, rect(40, 56, 70, 90, dy=1))]
    pred = [(S[6], 0, 0, rect(0, 30, 0, W)), (S[7], 2, 0, rect(30, 66, 0, W)), (S[8], 2, 0, rect(66, 96, 0, W)),
            (S[9], 3, 0, rect(22, 50, 11, 31, dx=3)), (S[10], 4, 0, rect(60, 85, 20, 70, dx=-2)), (S[11], 5, 0, rect(41, 56, 70, 91, dy=1)),
            (S[0], 3, 0, rect(2, 12, 140, 155))]
    return video(vid, T, gt, pred)


def scene_clean():
    return [street("v_a", 9), street("v_b", 10, shift=20), street("v_c", 12, shift=40)]


def scene_crowd_void():
    S = [seg_id(k + 60) for k in range(12)]
    gt = [(S[0], 0, 0, rect(0, 30, 0, W)), (S[1], 1, 0, rect(60, 96, 0, 120)),            # rows 30-60 and the right of the road: VOID
          (S[2], 3, 1, rect(30, 60, 0, 80)),                                                # a crowd of persons
          (S[3], 3, 0, rect(62, 90, 10, 40, dx=2)), (S[4], 4, 0, rect(5, 25, 100, 140))]
    pred = [(S[5], 0, 0, rect(0, 31, 0, W)), (S[6], 1, 0, rect(58, 96, 0, 118)),
            (S[7], 3, 0, rect(34, 58, 10, 60)),                                             # mostly on the crowd region: ignored
            (S[8], 5, 0, rect(35, 55, 100, 150)),                                           # mostly on VOID: ignored
            (S[9], 3, 0, rect(63, 90, 11, 41, dx=2)), (S[10], 4, 0, rect(5, 25, 60, 95)),  # a car in the wrong place
            (S[11], 3, 0, rect(40, 70, 70, 100))]                                           # half on the crowd, half elsewhere: a false alarm
    return [video("v_crowd", 9, gt, pred), street("v_d", 8, shift=90)]


def scene_enter_leave():
    S = [seg_id(k + 120) for k in range(12)]
    gt = [(S[0], 0, 0, rect(0, 40, 0, W)), (S[1], 1, 0, rect(40, 96, 0, W)),
          (S[2], 3, 0, rect(30, 60, 10, 40, dx=2, first=4)), (S[3], 4, 0, rect(50, 80, 90, 140, dx=-3, last=5)),
          (S[4], 5, 0, rect(10, 30, 60, 90))]
    pred = [(S[5], 0, 0, rect(0, 41, 0, W)), (S[6], 1, 0, rect(41, 96, 0, W)),
            (S[7], 3, 0, rect(30, 60, 11, 42, dx=2, first=3)), (S[8], 4, 0, rect(50, 80, 92, 140, dx=-3, last=6)),
            (S[9], 5, 0, rect(10, 31, 60, 90, last=7))]
    v = video("v_enter", 10, gt, pred)
    v["gt_info"][3] = [el for el in v["gt_info"][3] if el["id"] != S[4]]                    # pixels of an id this frame's record does not list
    return [v]


def scene_short():
    return [street("v_short", 5, shift=150), street("v_long", 9, shift=170)]


def scene_big_tables():
    gt, pred = [], []
    k = 0
    for gy in range(12):
        for gx in range(20):
            cat = (gy * 20 + gx) % 6
            gt.append((seg_id(300 + k), cat, 0, rect(gy * 8, gy * 8 + 8, gx * 8, gx * 8 + 8)))
            off = 1 if k % 3 else 5                                                         # every third cell is shifted beyond a match
            pred.append((seg_id(700 + k), cat if k % 7 else (cat + 1) % 6, 0, rect(gy * 8, gy * 8 + 8, gx * 8 + off, gx * 8 + 8 + off)))
            k += 1
    return [video("v_grid", 8, gt, pred)]


def _err_base():
    return [street("v_e", 4, shift=200)]


def scene_err_png_not_json():
    vs = _err_base()
    vs[0]["pred_info"][1] = vs[0]["pred_info"][1][1:]
    return vs


def scene_err_json_not_png():
    vs = _err_base()
    vs[0]["pred_info"][2].append({"id": seg_id(999), "category_id": 3, "iscrowd": 0, "area": 5})
    return vs


def scene_err_area_mismatch():
    vs = _err_base()
    vs[0]["pred_info"][0][2]["area"] += 1
    return vs


def scene_err_unknown_category():
    vs = _err_base()
    vs[0]["pred_info"][3][1]["category_id"] = 99
    return vs


def scene_err_size_mismatch():
    S = [seg_id(k + 230) for k in range(2)]
    return [video("v_size", 3, [(S[0], 0, 0, rect(0, 96, 0, W))], [(S[1], 0, 0, rect(0, 90, 0, 150))], pred_size=(90, 150))]


SCENES = {"clean": scene_clean, "crowd_void": scene_crowd_void, "enter_leave": scene_enter_leave, "short": scene_short,
          "big_tables": scene_big_tables, "err_png_not_json": scene_err_png_not_json, "err_json_not_png": scene_err_json_not_png,
          "err_area_mismatch": scene_err_area_mismatch, "err_unknown_category": scene_err_unknown_category,
          "err_size_mismatch": scene_err_size_mismatch}


def jsons_of(videos):
    gt = {"categories": CATEGORIES,
          "videos": [{"video_id": v["video_id"], "images": [{"file_name": n} for n in v["names"]]} for v in videos],
          "annotations": [{"video_id": v["video_id"], "annotations": [{"file_name": n, "segments_info": s} for n, s in zip(v["names"], v["gt_info"])]}
                          for v in videos]}
    pred = {"annotations": [{"video_id": v["video_id"], "annotations": [{"file_name": n, "segments_info": s} for n, s in zip(v["names"], v["pred_info"])]}
                            for v in videos]}
    return gt, pred


def ids_to_rgb(ids):
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


def write_tree(root, videos):
    gt_json, pred_json = jsons_of(videos)
    submit, truth = os.path.join(root, "submit"), os.path.join(root, "truth")
    for v in videos:
        for sub, key in ((os.path.join(truth, v["video_id"]), "gt"), (os.path.join(submit, "pan_pred", v["video_id"]), "pred")):
            os.makedirs(sub, exist_ok=True)
            for t, n in enumerate(v["names"]):
                Image.fromarray(ids_to_rgb(v[key][t])).save(os.path.join(sub, n))
    with open(os.path.join(submit, "pred.json"), "w") as f:
        json.dump(pred_json, f)
    gt_file = os.path.join(root, "gt.json")
    with open(gt_file, "w") as f:
        json.dump(gt_json, f)
    return submit, truth, gt_file, gt_json, pred_json


def load_reference():
    np.bool = bool                                                   # STQuality uses the removed alias
    sys.path.insert(0, REF_EVAL)

    def by_path(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF_EVAL, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    stq_lib = by_path("eval_stquality_vps")
    return by_path("eval_vpq_vps"), by_path("eval_stq_vps"), stq_lib


def run_reference(mods, submit, truth, gt_file):
    vpq, stq, stq_lib = mods
    kept = {"vpq": [], "stq": []}
    pq_average, result = vpq.PQStat.pq_average, stq_lib.STQuality.result

    def keep_pq(self, categories, isthing):
        r = pq_average(self, categories, isthing)
        kept["vpq"].append((isthing, r))
        return r

    def keep_stq(self):
        r = result(self)
        kept["stq"].append(r)
        return r
    vpq.PQStat.pq_average, stq_lib.STQuality.result = keep_pq, keep_stq
    argv = sys.argv
    try:
        sys.argv = ["eval", "--submit_dir", submit, "--truth_dir", truth, "--pan_gt_json_file", gt_file]
        vpq.main()
        stq.main()
    finally:
        sys.argv = argv
        vpq.PQStat.pq_average, stq_lib.STQuality.result = pq_average, result
    return kept


def main():
    mods = load_reference()
    os.makedirs(GOLDEN, exist_ok=True)
    seen = {"Things": np.zeros(3, np.int64), "Stuff": np.zeros(3, np.int64)}
    for name, make in SCENES.items():
        videos = make()
        with tempfile.TemporaryDirectory() as root:
            submit, truth, gt_file, gt_json, pred_json = write_tree(root, videos)
            rec = {"video_ids": np.array([v["video_id"] for v in videos]), "gt_json": np.array(json.dumps(gt_json)),
                   "pred_json": np.array(json.dumps(pred_json))}
            for v in videos:
                rec["gt_" + v["video_id"]] = v["gt"]
                rec["pred_" + v["video_id"]] = v["pred"]
            if name.startswith("err_"):
                try:
                    run_reference(mods, submit, truth, gt_file)
                except (KeyError, AssertionError) as e:
                    rec["error"] = np.array(type(e).__name__)
                assert "error" in rec, f"{name}: the reference did not raise"
            else:
                kept = run_reference(mods, submit, truth, gt_file)    # the reference runs to the end: no iou or area assertion
                assert len(kept["vpq"]) == 15 and len(kept["stq"]) == 1
                for i, nframes in enumerate((1, 2, 4, 6, 8)):
                    (_, (all_avg, per_class)), (_, (th_avg, _)), (_, (st_avg, _)) = kept["vpq"][3 * i:3 * i + 3]
                    cats = list(per_class)
                    rec[f"vpq{nframes}_cats"] = np.array(cats, dtype=np.int64)
                    rec[f"vpq{nframes}_iou"] = np.array([per_class[c]["iou"] for c in cats], dtype=np.float64)
                    for k in ("tp", "fp", "fn"):
                        rec[f"vpq{nframes}_{k}"] = np.array([per_class[c][k] for c in cats], dtype=np.int64)
                    rec[f"vpq{nframes}_avg"] = np.array([[a["pq"], a["sq"], a["rq"], a["n"]] for a in (all_avg, th_avg, st_avg)], dtype=np.float64)
                    for c in cats:
                        seen["Things" if CATEGORIES[c]["isthing"] else "Stuff"] += [per_class[c]["tp"], per_class[c]["fp"], per_class[c]["fn"]]
                files = sorted(f for f in os.listdir(submit) if f.endswith(".txt"))
                assert files == sorted(["vpq-0.txt", "vpq-5.txt", "vpq-15.txt", "vpq-25.txt", "vpq-35.txt", "vpq-final.txt", "stq-final.txt"])
                rec["file_names"] = np.array(files)
                rec["file_texts"] = np.array([open(os.path.join(submit, f)).read() for f in files])
                r = kept["stq"][0]
                rec["stq"] = np.array([r["STQ"], r["AQ"], r["IoU"]], dtype=np.float64)
                for k in ("STQ_per_seq", "AQ_per_seq", "IoU_per_seq", "Length_per_seq"):
                    rec[k.lower()] = np.array(r[k], dtype=np.float64)
                if name == "crowd_void":                             # the two ignored predictions are what the scene says they are
                    v = videos[0]
                    crowd = v["gt"] == v["gt_info"][0][2]["id"]
                    on_crowd, on_void = v["pred"] == v["pred_info"][0][2]["id"], v["pred"] == v["pred_info"][0][3]["id"]
                    assert v["gt_info"][0][2]["iscrowd"] == 1 and (crowd & on_crowd).sum() / on_crowd.sum() > 0.5
                    assert ((v["gt"] == 0) & on_void).sum() / on_void.sum() > 0.5
                    # and the reference treats them so: alone, this video has no dog but the one on VOID, which is neither hit nor
                    # false alarm; with the crowd flag taken away, the person on the crowd becomes a false alarm
                    alone = run_reference(mods, *write_tree(os.path.join(root, "alone"), [v])[:3])
                    plain = dict(v, gt_info=[[dict(el, iscrowd=0) for el in fr] for fr in v["gt_info"]])
                    uncrowded = run_reference(mods, *write_tree(os.path.join(root, "plain"), [plain])[:3])
                    for i in range(5):
                        a, u = alone["vpq"][3 * i][1][1], uncrowded["vpq"][3 * i][1][1]
                        assert a[5]["tp"] == 0 and a[5]["fp"] == 0 and a[3]["fp"] < u[3]["fp"], (i, a, u)
        path = os.path.join(GOLDEN, f"g26_vps_eval_{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, os.path.getsize(path), "bytes", rec.get("error", ""))
    assert (seen["Things"] > 0).all() and (seen["Stuff"] > 0).all(), seen
    print("tp / fp / fn seen:", seen)


if __name__ == "__main__":
    main()
