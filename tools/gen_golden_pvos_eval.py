"""Golden fixtures of the VIPOSeg panoptic-VOS scoring (tests/golden/g30_pvos_eval_*.npz): the reference's own `eval_iou` and the
file-writing body of `PVOSEvaluator.evaluate` (univs/evaluation/pvos_evaluation.py) over `boundary_iou`
(univs/evaluation/eval_utils_viposeg.py), run on small synthetic VIPOSeg trees in a temporary directory, and `mask_to_boundary` called
directly for the operator-level cases.

The evaluator object is made without its constructor (which needs detectron2's MetadataCatalog) and handed the output directory and the
split's path; `evaluate` then runs unmodified.  `eval_iou` is wrapped to keep what it returns, and its per-object lists are read from its
frame when it returns; nothing else of the reference runs differently.  Stand-ins: detectron2's inert bases, panopticapi and tqdm from
`oracle.ref_harness.ref_evaluators()`, and OpenCV, which is absent here, by its documented rules restated with numpy and SciPy:

    cv2.copyMakeBorder(src, t, b, l, r, cv2.BORDER_CONSTANT, value=v)   np.pad(src, ((t, b), (l, r)), constant_values=v)
    cv2.erode(src, ones 3 x 3, iterations=n)                             scipy.ndimage.binary_erosion(src, structure=kernel, iterations=n,
                                                                         border_value=1)   (erode's default border never erodes)

so the fixtures pin everything the reference does EXCEPT OpenCV's own code.

A scene fixture holds the videos (`seqs`: those of Annotations_gt, `res_seqs`: those with results), per video the id maps and file names
(`gt_<v>` / `gt_names_<v>`, `pred_<v>` / `pred_names_<v>`, `ann_<v>` / `ann_names_<v>`: the reference frames that let objects enter),
obj_class.json as text, and for a scene the reference scores: the per-object values in append order (`<group>_miou`, `<group>_biou`,
`decay_k` / `decay_n` / `decay_v`: the keys of the decay table with data, their lengths and their values back to back), the returned
dictionary (`keys`, `values`) and the text of pvos-ious.txt.  An error scene holds the exception's type name.
`g30_pvos_eval_operators.npz` holds one pair of 64 x 96 stacks and, for d in (1, 2, 5, 8, 18, 29), the six counts of every id and frame
from the parts of `boundary_iou`.  `g30_pvos_eval_classes.npz` holds the reference's class lists and video names, which this tool
asserts equal to the tuples of univs_amd/evaluation/pvos.py.

Scenes: `clean` (3 videos, objects of all four groups, one of the 23 named videos with a class-98 object and one other); `enter_leave`
(objects entering at later reference frames, an object absent for some frames on either side and on both); `duplicate_ids` (an id in
two reference frames); `edges` (objects on the last row and column, single pixels, a full-frame object, id 255); `fewer_results` (two
results for three videos, the ground-truth list paired by index); `unlisted_class`; `empty_group` (a NaN mean); `many_objects` (64
objects entering 8 at a time, so the fit's `k < 60` matters); `wide` (120 x 214, d = 5); and the error scenes `err_frame_count`,
`err_missing_class`, `err_80_objects`, `err_size_mismatch`.  Every scored scene has a non-degenerate decay fit (asserted here).

    python tools/gen_golden_pvos_eval.py     # needs the reference tree (dev container only)
"""
import importlib.util
import json
import logging
import os
import sys
import tempfile
import types

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
from oracle.ref_harness import REF_ROOT, ref_evaluators  # noqa: E402  (UNIVS_REFERENCE_ROOT)
from tools.gen_golden_davis_eval import jitter, paint  # noqa: E402

DS = (1, 2, 5, 8, 18, 29)
GROUPS = ("thing_seen", "thing_unseen", "stuff_seen", "stuff_unseen")
MAX_BYTES = 14885                                                    # the largest g28 fixture
NAMED = "187_WUZUSD4477I"                                            # one of the 23 "other machine" videos
# one class of each group: thing seen / thing unseen / stuff seen / stuff unseen
TS, TU, SS, SU = 60, 102, 28, 9


# ------------------------------------------------------------------------------------------------------------------------------------
# synthetic videos
# ------------------------------------------------------------------------------------------------------------------------------------
def video(name, gt, pred, ann, classes, pred_names=None):
    """`ann`: {frame index: id map of the reference frame}; `classes`: {id: class}."""
    names = ["%05d.png" % t for t in range(len(gt))]
    return {"name": name, "gt": gt, "gt_names": names, "pred": pred, "pred_names": names if pred_names is None else pred_names,
            "ann": np.stack([ann[i] for i in sorted(ann)]), "ann_names": [names[i] for i in sorted(ann)],
            "classes": {str(k): v for k, v in classes.items()}}


def panoptic(T, H, W, objects, stuff=((1, 0.5),)):
    """A label map without holes: horizontal bands of stuff ids `stuff` = ((id, share of the height), ...), `objects` painted over."""
    out = np.zeros((T, H, W), np.uint8)
    y = 0
    for k, share in stuff:
        y1 = H if (k, share) == tuple(stuff[-1]) else min(H, y + int(round(share * H)))
        out[:, y:y1] = k
        y = y1
    fg = paint(T, H, W, objects)
    return np.where(fg > 0, fg, out)


def only(ids, m):
    return np.where(np.isin(m, list(ids)), m, 0).astype(np.uint8)


THREE = [(3, 12, 14, 7, 9, 0.5, 1.5, 1.0), (4, 28, 30, 6, 6, -0.5, 1.0, 1.5), (5, 20, 44, 5, 8, 0.3, -1.2, 0.8)]
BANDS = ((1, 0.4), (2, 0.6))


def scene_clean():
    H, W = 40, 56
    ga = panoptic(6, H, W, THREE, BANDS)
    a = video(NAMED, ga, panoptic(6, H, W, jitter(THREE, 1), ((1, 0.45), (2, 0.55))), {0: ga[0]}, {1: 98, 2: SU, 3: TS, 4: TU, 5: TS})
    gb = panoptic(5, H, W, THREE[:2], BANDS)
    b = video("20_abc", gb, panoptic(5, H, W, jitter(THREE[:2], 2, 2.5, 2.0), BANDS), {0: gb[0]}, {1: 98, 2: SS, 3: TU, 4: TS})
    gc = panoptic(4, H, W, THREE[:1], ((1, 1.0),))
    c = video("7_xyz", gc, panoptic(4, H, W, jitter(THREE[:1], 3), ((1, 1.0),)), {0: gc[0]}, {1: SS, 3: TS})
    return dict(videos=[a, b, c])


def scene_enter_leave():
    H, W, T = 40, 56, 9
    gt = panoptic(T, H, W, THREE, BANDS)
    pred = panoptic(T, H, W, jitter(THREE, 4), BANDS)
    gt[3:5][gt[3:5] == 4] = 2                                        # object 4 leaves the gt for two frames
    pred[4:6][pred[4:6] == 4] = 2                                    # ... and the result for two, one of them the same
    pred[7][pred[7] == 3] = 1
    ann = {0: only((1, 2), gt[0]), 2: only((3,), gt[2]), 5: only((4, 5), gt[5])}
    return dict(videos=[video("31_enter", gt, pred, ann, {1: SS, 2: SU, 3: TS, 4: TU, 5: TU})])


def scene_duplicate_ids():
    H, W, T = 40, 56, 6
    gt = panoptic(T, H, W, THREE[:2], BANDS)
    pred = panoptic(T, H, W, jitter(THREE[:2], 5), BANDS)
    ann = {0: only((1, 3), gt[0]), 2: only((2, 3, 4), gt[2]), 3: only((1,), gt[3])}          # 3 and 1 come twice
    return dict(videos=[video("44_twice", gt, pred, ann, {1: SS, 2: SU, 3: TS, 4: TU})])


def scene_edges():
    H, W, T = 41, 57, 6
    gt = np.zeros((T, H, W), np.uint8)
    pred = np.zeros((T, H, W), np.uint8)
    gt[:, H - 3:, 4:12] = 1                                          # on the last row
    gt[:, 5:14, W - 2:] = 2                                          # on the last column
    gt[:, H - 1, W - 1] = 3                                          # the bottom-right pixel alone
    gt[:, 10, 10] = 4                                                # a single pixel
    gt[:, 0, :6] = 255                                               # id 255 on the first row
    pred[:, H - 2:, 5:13] = 1
    pred[:, 4:14, W - 1:] = 2
    pred[:, H - 1, W - 1] = 3
    pred[:, 10, 11] = 4
    pred[:, 0:2, :5] = 255
    ann0 = gt[0].copy()
    gt[3], pred[3] = 1, 1                                            # a full-frame object on both sides
    gt[4] = 2                                                        # ... on one side
    pred[5] = 0                                                      # an empty result
    a = video("52_edges", gt, pred, {0: ann0}, {1: SS, 2: SU, 3: TS, 4: TU, 255: TS})
    gb = panoptic(4, 40, 56, THREE[:1], ((1, 1.0),))
    b = video("9_more", gb, panoptic(4, 40, 56, jitter(THREE[:1], 6), ((1, 1.0),)), {0: gb[0]}, {1: SS, 3: TU})
    return dict(videos=[a, b])


def scene_fewer_results():
    """Results for the first and the third of three videos: the reference keeps the references of those two, and pairs them by index
    with the FIRST TWO ground-truth folders, so the second video's labels are scored against the third's results and references."""
    H, W = 40, 56
    names = ("10_a", "20_b", "30_c")
    out = []
    for n, (name, seed) in enumerate(zip(names, (7, 8, 9))):
        objs = [(k, cy + 2 * n, cx + 3 * n, ry, rx, vy, vx, wob) for (k, cy, cx, ry, rx, vy, vx, wob) in THREE[:2 + (n == 0)]]
        g = panoptic(5, H, W, objs, BANDS)
        out.append(video(name, g, panoptic(5, H, W, jitter(objs, seed), BANDS), {0: g[0]}, {1: SS, 2: SU, 3: TS, 4: TU, 5: TS}))
    return dict(videos=out, results=("10_a", "30_c"))


def scene_unlisted_class():
    s = scene_clean()
    s["videos"] = s["videos"][:2]
    s["videos"][0]["classes"]["5"] = 124                             # in none of the four lists
    s["videos"][1]["classes"]["4"] = 200
    return s


def scene_empty_group():
    s = scene_clean()
    for v in s["videos"]:
        v["classes"] = {k: (TS if c == TU else c) for k, c in v["classes"].items()}     # no unseen thing
    return s


def scene_many_objects():
    """64 objects, 8 more after each of the first 8 frames: the decay table has data at 8, 16, .., 64, the fit takes those below 60."""
    H, W, T = 40, 56, 10
    gt = np.zeros((T, H, W), np.uint8)
    for k in range(64):                                              # an 8 x 8 grid of 5 x 7 cells
        y, x = 5 * (k // 8), 7 * (k % 8)
        gt[:, y:y + 5, x:x + 7] = k + 1
    rng = np.random.default_rng(12)
    pred = gt.copy()
    for t in range(T):
        pred[t] = np.roll(gt[t], (int(rng.integers(0, 2)), int(rng.integers(0, 3))), axis=(0, 1))
    ann = {t: only(range(8 * t + 1, 8 * t + 9), gt[t]) for t in range(8)}
    classes = {k + 1: (TS, TU, SS, SU)[k % 4] for k in range(64)}
    return dict(videos=[video("64_many", gt, pred, ann, classes)])


def scene_wide():
    H, W = 120, 214
    objs = [(3, 40, 60, 20, 30, 2, 5, 3), (4, 80, 150, 18, 22, -2, -4, 2)]
    gt = panoptic(4, H, W, objs, BANDS)
    ann = {0: only((1, 2, 3), gt[0]), 1: only((4,), gt[1])}
    return dict(videos=[video("77_wide", gt, panoptic(4, H, W, jitter(objs, 10, 3.0, 2.0), BANDS), ann, {1: SS, 2: SU, 3: TS, 4: TU})])


def scene_err_frame_count():
    s = scene_clean()
    v = s["videos"][1]
    v["pred"], v["pred_names"] = v["pred"][:-1], v["pred_names"][:-1]
    return dict(videos=s["videos"], error=AssertionError)


def scene_err_missing_class():
    s = scene_clean()
    del s["videos"][1]["classes"]["4"]
    return dict(videos=s["videos"], error=KeyError)


def scene_err_80_objects():
    H, W, T = 40, 56, 3
    gt = np.zeros((T, H, W), np.uint8)
    for k in range(80):                                              # a 10 x 8 grid of 4 x 7 cells
        y, x = 4 * (k // 8), 7 * (k % 8)
        gt[:, y:y + 4, x:x + 7] = k + 1
    return dict(videos=[video("80_many", gt, gt.copy(), {0: gt[0]}, {k + 1: TS for k in range(80)})], error=KeyError)


def scene_err_size_mismatch():
    s = scene_clean()
    v = s["videos"][2]
    v["pred"] = np.ascontiguousarray(v["pred"][:, :-2, :-4])
    return dict(videos=s["videos"], error=ValueError)


SCENES = {"clean": scene_clean, "enter_leave": scene_enter_leave, "duplicate_ids": scene_duplicate_ids, "edges": scene_edges,
          "fewer_results": scene_fewer_results, "unlisted_class": scene_unlisted_class, "empty_group": scene_empty_group,
          "many_objects": scene_many_objects, "wide": scene_wide, "err_frame_count": scene_err_frame_count,
          "err_missing_class": scene_err_missing_class, "err_80_objects": scene_err_80_objects,
          "err_size_mismatch": scene_err_size_mismatch}


def operator_stacks():
    """One pair of 64 x 96 stacks: d = 29 reaches across the whole image, so every pixel is boundary there."""
    H, W, T = 64, 96, 3
    objs = [(3, 20, 25, 12, 16, 3, 6, 2), (4, 44, 60, 10, 14, -2, 4, 2), (5, 60, 90, 6, 8, 0, 0, 1)]
    gt = panoptic(T, H, W, objs, BANDS)
    gt[:, 0, 0:10] = 5
    pred = panoptic(T, H, W, jitter(objs, 11, 4.0, 3.0) + [(6, 8, 80, 5, 7, 2, -3, 1)], ((1, 0.45), (2, 0.55)))
    pred[:, H - 1, W - 6:] = 6
    pred[2] = np.where(pred[2] == 4, 2, pred[2])                     # id 4 absent from the result of the last frame
    return gt, pred


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------
def load_reference():
    """The reference's pvos_evaluation module, imported from its file with the stand-ins of the module docstring."""
    import scipy.ndimage
    ref_evaluators()                                                 # detectron2's inert bases, panopticapi, tqdm, `_ref_evaluation`
    cv2 = types.ModuleType("cv2")
    cv2.BORDER_CONSTANT = 0
    cv2.copyMakeBorder = lambda src, top, bottom, left, right, borderType, value=0: np.pad(src, ((top, bottom), (left, right)),
                                                                                             constant_values=value)
    cv2.erode = lambda src, kernel, iterations=1: scipy.ndimage.binary_erosion(src, structure=kernel, iterations=iterations,
                                                                               border_value=1).astype(src.dtype)
    sys.modules["cv2"] = cv2
    name = "_ref_evaluation.pvos_evaluation"
    spec = importlib.util.spec_from_file_location(name, f"{REF_ROOT}/univs/evaluation/pvos_evaluation.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def write_tree(root, scene):
    """VIPOSeg split + result directory of a scene -> (data_path, output_dir).  Shared with tests/pvos_eval_cases.py in layout only."""
    data, out = os.path.join(root, "VIPOSeg", "valid"), os.path.join(root, "out")
    os.makedirs(os.path.join(out, "Annotations"), exist_ok=True)
    results = scene.get("results", tuple(v["name"] for v in scene["videos"]))
    for v in scene["videos"]:
        todo = [(os.path.join(data, "Annotations_gt", v["name"]), v["gt"], v["gt_names"]),
                (os.path.join(data, "Annotations", v["name"]), v["ann"], v["ann_names"])]
        if v["name"] in results:
            todo.append((os.path.join(out, "Annotations", v["name"]), v["pred"], v["pred_names"]))
        for sub, maps, names in todo:
            os.makedirs(sub, exist_ok=True)
            for m, n in zip(maps, names):
                Image.fromarray(m).save(os.path.join(sub, n), format="PNG")
    with open(os.path.join(data, "obj_class.json"), "w") as f:
        f.write(obj_class_text(scene))
    return data, out


def obj_class_text(scene):
    return json.dumps({v["name"]: v["classes"] for v in scene["videos"]})


def run_reference(ref, data, out):
    """`PVOSEvaluator.evaluate` of the reference -> (returned dictionary, the locals of `eval_iou` at its return, text of pvos-ious.txt)."""
    kept = {}
    eval_iou = ref.eval_iou

    def keep_res(*a, **k):
        def prof(frame, event, arg):
            if event == "return" and frame.f_code is eval_iou.__code__:
                kept["locals"] = dict(frame.f_locals)
        sys.setprofile(prof)
        try:
            kept["res"] = eval_iou(*a, **k)
        finally:
            sys.setprofile(None)
        return kept["res"]
    ref.eval_iou = keep_res
    try:
        e = object.__new__(ref.PVOSEvaluator)
        e._output_dir, e.data_path, e.eval_decay, e.dataset_name = out, data, True, "viposeg_valid"
        e._logger = logging.getLogger("gen_golden_pvos_eval")
        e.reset()
        e.process([{}], {})
        e.evaluate()
    finally:
        ref.eval_iou = eval_iou
    with open(os.path.join(out, "pvos-ious.txt"), newline="") as f:
        return kept["res"], kept["locals"], f.read()


def save(name, rec):
    path = os.path.join(GOLDEN, f"g30_pvos_eval_{name}.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= MAX_BYTES, f"{name}: {os.path.getsize(path)} bytes"
    return os.path.getsize(path)


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    ref = load_reference()
    from _ref_evaluation.eval_utils_viposeg import VIPOSeg, mask_to_boundary
    from univs_amd.evaluation import pvos as ours

    vp = VIPOSeg()
    lists = {"thing_seen": vp.thing_seen_class, "thing_unseen": vp.thing_unseen_class, "stuff_seen": vp.stuff_seen_class,
             "stuff_unseen": vp.stuff_unseen_class}
    assert tuple(vp.thing_seen_class) == ours.THING_SEEN_CLASS and tuple(vp.thing_unseen_class) == ours.THING_UNSEEN_CLASS
    assert tuple(vp.stuff_seen_class) == ours.STUFF_SEEN_CLASS and tuple(vp.stuff_unseen_class) == ours.STUFF_UNSEEN_CLASS
    assert tuple(vp.other_machine_videos) == ours.OTHER_MACHINE_VIDEOS and vp.other_machine_cl == ours.OTHER_MACHINE_CLASS
    assert NAMED in vp.other_machine_videos and 124 not in sum(lists.values(), []) and 200 not in sum(lists.values(), [])
    print("classes", save("classes", dict({k: np.array(v) for k, v in lists.items()}, other_machine_videos=np.array(vp.other_machine_videos),
                                          other_machine_class=np.array(vp.other_machine_cl))), "bytes")

    gt, pred = operator_stacks()
    K, (T, H, W) = 6, gt.shape
    rec = {"gt": gt, "pred": pred, "K": np.array(K), "ds": np.array(DS)}
    diag = np.sqrt(H ** 2 + W ** 2)
    for d in DS:
        c = np.zeros((T, K, 6), np.int64)
        for t in range(T):
            for k in range(1, K + 1):
                mask_gt, mask_pred = gt[t] == k, pred[t] == k
                gb = mask_to_boundary(mask_gt.astype(np.uint8), d / diag)      # (dilation = int(round(ratio * diagonal)) = d)
                pb = mask_to_boundary(mask_pred.astype(np.uint8), d / diag)
                c[t, k - 1] = (np.sum(mask_gt & mask_pred), np.sum(mask_gt), np.sum(mask_pred), ((gb * pb) > 0).sum(), (gb > 0).sum(),
                               (pb > 0).sum())
        assert int(round(d / diag * diag)) == d
        rec[f"counts_d{d}"] = c.astype(np.int32)
    print("operators", save("operators", rec), "bytes")

    for name, make in SCENES.items():
        scene = make()
        error = scene.get("error")
        results = scene.get("results", tuple(v["name"] for v in scene["videos"]))
        rec = {"seqs": np.array([v["name"] for v in scene["videos"]]), "res_seqs": np.array(results), "obj_class": np.array(obj_class_text(scene))}
        for v in scene["videos"]:
            for k in ("gt", "pred", "ann"):
                rec[f"{k}_{v['name']}"], rec[f"{k}_names_{v['name']}"] = v[k], np.array(v[k + "_names"])
        with tempfile.TemporaryDirectory() as root:
            data, out = write_tree(root, scene)
            if error is not None:
                try:
                    run_reference(ref, data, out)
                except error as e:
                    rec["error"] = np.array(type(e).__name__)
                assert "error" in rec, f"{name}: the reference did not raise"
            else:
                res, loc, text = run_reference(ref, data, out)
                for g in GROUPS:
                    rec[f"{g}_miou"] = np.array(loc[f"{g}_miou_list"], dtype=np.float64)
                    rec[f"{g}_biou"] = np.array(loc[f"{g}_biou_list"], dtype=np.float64)
                table = {k: v for k, v in loc["iou_decay_dict"].items() if v != []}
                rec["decay_k"] = np.array(list(table), dtype=np.int64)
                rec["decay_n"] = np.array([len(v) for v in table.values()], dtype=np.int64)
                rec["decay_v"] = np.array([x for v in table.values() for x in v], dtype=np.float64)
                fitted = [np.mean(v) for k, v in table.items() if k < 60]
                assert len(fitted) >= 2 and min(fitted) > 0, f"{name}: degenerate decay fit {fitted}"
                assert np.isfinite(res["decay"]), name
                rec["keys"] = np.array(list(res))
                rec["values"] = np.array(list(res.values()), dtype=np.float64)
                rec["text"] = np.array(text)
        print(name, save(name, rec), "bytes", rec.get("error", ""), rec.get("text", ""), sep="\n  ")


if __name__ == "__main__":
    main()
