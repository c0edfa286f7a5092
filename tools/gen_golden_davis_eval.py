"""Golden fixtures of the DAVIS scoring (tests/golden/g28_davis_eval_*.npz): the reference's own `evaluate_davis` and the file-writing
body of `DAVISEvaluator.evaluate` (univs/evaluation/vos_davis_evaluation.py) over its vendored davis2017 package, run on small
synthetic DAVIS trees in a temporary directory, and `db_eval_iou` / `db_eval_boundary` called directly for the operator-level cases.

The evaluator object is made without its constructor (which needs detectron2's MetadataCatalog) and handed the reference's own `DAVIS`
dataset object, the task, the metrics and the output directory; `evaluate` then runs unmodified.  `evaluate_davis` and the two
`_evaluate_*` functions are wrapped to keep what they return; nothing else of the reference runs differently.  Stand-ins: detectron2's
inert bases from `oracle.ref_harness.ref_evaluators()`, an empty `pycocotools.mask` (imported, never called), and the two image
libraries that are absent here, by their documented rules restated with SciPy:

    skimage.morphology.disk(r)   (X^2 + Y^2 <= r^2) on arange(-r, r + 1)
    cv2.dilate(src, kernel)      scipy.ndimage.binary_dilation(src, structure=kernel, border_value=0)

so the fixtures pin everything the reference does EXCEPT OpenCV's and scikit-image's own code.

Each scene fixture holds the id maps and file names of every sequence (`gt_<seq>`, `gt_names_<seq>`, `pred_<seq>`, `pred_names_<seq>`),
the task / resolution / metrics, and for a scene the reference scores: the per-frame tables `j_<seq>` / `f_<seq>`, the returned
dictionary (`<m>_M`, `<m>_R`, `<m>_D`, `<m>_keys`, `<m>_per_object`) and the text of davis-metrics.txt.  An error scene holds the
exception's type name.  `g28_davis_eval_operators.npz` holds one pair of 64 x 96 stacks and, for r in (1, 2, 5, 8, 18) with and
without the void mask, the J and F of every (gt object, result object, frame).

Scenes: `semi_clean` (12, 9 and 5 frames, 1-3 objects, moving and deforming); `semi_fewer_results` (a padded empty result object, a
gt object absent in some frames); `unsup_clean` (6 proposals against 3 objects in permuted order, void regions that cut through object
boundaries); `unsup_20` (exactly 20 proposals); `edges` (objects on the last row, the last column and the bottom-right pixel,
single-pixel objects, a frame where both sides are empty, one where one side is); `long_300` (300 frames of 12 x 16: the uint8 wrap of
`db_statistics`); `radius_2` (120 x 214); and the error scenes `err_missing_frame`, `err_too_many_objects`, `err_21_proposals`,
`err_size_mismatch`, `err_unsup_single_metric`.

    python tools/gen_golden_davis_eval.py     # needs the reference tree (dev container only)
"""
import importlib.util
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

RADII = (1, 2, 5, 8, 18)


# ------------------------------------------------------------------------------------------------------------------------------------
# synthetic sequences
# ------------------------------------------------------------------------------------------------------------------------------------
def paint(T, H, W, objects):
    """uint8 [T, H, W]: `objects` = [(id, cy, cx, ry, rx, vy, vx, wobble)], ellipses drawn in order, moving by (vy, vx) per frame and
    breathing by `wobble` pixels."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        for (k, cy, cx, ry, rx, vy, vx, wob) in objects:
            a, b = ry + wob * np.sin(0.9 * t), rx + wob * np.cos(0.7 * t)
            out[t][((yy - cy - vy * t) / max(a, 0.5)) ** 2 + ((xx - cx - vx * t) / max(b, 0.5)) ** 2 <= 1.0] = k
    return out


def jitter(objects, seed, shift=1.5, grow=1.0):
    rng = np.random.default_rng(seed)
    return [(k, cy + rng.uniform(-shift, shift), cx + rng.uniform(-shift, shift), ry + rng.uniform(-grow, grow), rx + rng.uniform(-grow, grow),
             vy, vx, wob) for (k, cy, cx, ry, rx, vy, vx, wob) in objects]


def seq(name, gt, pred, pred_names=None):
    names = ["%05d.png" % t for t in range(len(gt))]
    return {"name": name, "gt": gt, "gt_names": names, "pred": pred, "pred_names": names if pred_names is None else pred_names}


THREE = [(1, 12, 14, 7, 9, 0.5, 1.5, 1.0), (2, 28, 30, 6, 6, -0.5, 1.0, 1.5), (3, 20, 44, 5, 8, 0.3, -1.2, 0.8)]


def scene_semi_clean():
    H, W = 40, 56
    a = seq("bear", paint(12, H, W, THREE), paint(12, H, W, jitter(THREE, 1)))
    two = THREE[:2]
    b = seq("camel", paint(9, H, W, two), paint(9, H, W, jitter(two, 2, 2.5, 2.0)))
    one = [(1, 18, 20, 9, 12, 0.0, 2.0, 2.0)]
    c = seq("dog", paint(5, H, W, one), paint(5, H, W, jitter(one, 3)))
    return dict(task="semi-supervised", seqs=[a, b, c])


def scene_semi_fewer_results():
    H, W = 40, 56
    gt = paint(10, H, W, THREE)
    gt[3:6][gt[3:6] == 2] = 0                                        # object 2 leaves for three frames
    pred = paint(10, H, W, jitter(THREE[:2], 4))                     # no result for object 3: a padded empty mask
    pred[7][pred[7] == 1] = 0
    return dict(task="semi-supervised", seqs=[seq("goat", gt, pred)])


def scene_unsup_clean():
    H, W = 40, 56
    gt = paint(8, H, W, THREE)
    gt[:, :, 16:19] = 255                                            # void stripes through the objects' boundaries
    gt[:, 24:26, :] = 255
    gt[2:5, 5:15, 40:50] = 255
    perm = {1: 4, 2: 1, 3: 6}
    objs = [(perm[k], *rest) for (k, *rest) in jitter(THREE, 5)]
    extra = [(2, 34, 8, 3, 4, 0, 0.5, 0.5), (3, 6, 48, 3, 3, 0.2, 0, 0.3), (5, 30, 46, 4, 3, 0, -0.5, 0.4)]
    pred = paint(8, H, W, extra + objs)
    return dict(task="unsupervised", seqs=[seq("horse", gt, pred), seq("bear", paint(4, H, W, THREE[:1]), paint(4, H, W, jitter(THREE[:2], 6)))])


def scene_unsup_20():
    H, W = 32, 48
    gt = paint(5, H, W, [(1, 10, 12, 6, 8, 0.5, 1, 1), (2, 22, 32, 5, 7, 0, -1, 1)])
    gt[:, 14:16, :] = 255
    pred = np.zeros((5, H, W), np.uint8)
    for k in range(20):                                              # a 4 x 5 grid of proposals, two of them the objects
        y, x = 1 + 8 * (k // 5), 1 + 9 * (k % 5)
        pred[:, y:y + 6, x:x + 7] = k + 1
    pred[paint(5, H, W, jitter([(1, 10, 12, 6, 8, 0.5, 1, 1)], 7)) == 1] = 13
    pred[paint(5, H, W, jitter([(2, 22, 32, 5, 7, 0, -1, 1)], 8)) == 2] = 4
    return dict(task="unsupervised", seqs=[seq("pigs", gt, pred)])


def scene_edges():
    H, W, T = 24, 31, 7
    gt = np.zeros((T, H, W), np.uint8)
    pred = np.zeros((T, H, W), np.uint8)
    gt[:, H - 3:, 4:12] = 1                                          # on the last row
    gt[:, 5:14, W - 2:] = 2                                          # on the last column
    gt[:, H - 1, W - 1] = 3                                          # the bottom-right pixel alone
    gt[:, 10, 10] = 4                                                # a single pixel
    gt[:, 0, :6] = 5                                                 # on the first row
    gt[:, 2:5, 20:23] = 255
    pred[:, H - 2:, 5:13] = 1
    pred[:, 4:14, W - 1:] = 2
    pred[:, H - 1, W - 1] = 3
    pred[:, 10, 11] = 4
    pred[:, 0:2, :5] = 5
    pred[:, 16, 16] = 6
    gt[3] = 0                                                        # both sides empty
    pred[3] = 0
    gt[4] = 0                                                        # the gt empty
    pred[5] = 0                                                      # the result empty
    gt[6, gt[6] == 255] = 0
    gt[6, :, 7] = 255                                                # a void column through object 1
    return dict(task="unsupervised", seqs=[seq("edges", gt, pred)])


def scene_long_300():
    H, W, T = 12, 16, 300
    objs = [(1, 5, 3, 3, 3, 0.0, 0.03, 1.0), (2, 8, 11, 2, 3, -0.01, -0.02, 0.8)]
    gt = paint(T, H, W, objs)
    pred = paint(T, H, W, jitter(objs, 9, 0.8, 0.5))
    for t in range(0, T, 7):                                         # a score that decays and flickers
        pred[t][pred[t] == 2] = 0
    pred[200:, :, :4][pred[200:, :, :4] == 1] = 0
    return dict(task="semi-supervised", seqs=[seq("long", gt, pred)])


def scene_radius_2():
    H, W = 120, 214
    objs = [(1, 40, 60, 20, 30, 2, 5, 3), (2, 80, 150, 18, 22, -2, -4, 2)]
    return dict(task="semi-supervised", seqs=[seq("wide", paint(5, H, W, objs), paint(5, H, W, jitter(objs, 10, 3.0, 2.0)))])


def scene_err_missing_frame():
    s = scene_semi_clean()["seqs"][2]
    s["pred"], s["pred_names"] = s["pred"][[0, 1, 3, 4]], [s["pred_names"][i] for i in (0, 1, 3, 4)]
    return dict(task="semi-supervised", seqs=[s], error=SystemExit)


def scene_err_too_many_objects():
    s = scene_semi_clean()["seqs"][2]
    s["pred"][2, 0:3, 0:3] = 2
    return dict(task="semi-supervised", seqs=[s], error=SystemExit)


def scene_err_21_proposals():
    s = scene_unsup_20()["seqs"][0]
    s["pred"][1, 30:32, 40:44] = 21
    return dict(task="unsupervised", seqs=[s], error=SystemExit)


def scene_err_size_mismatch():
    s = scene_semi_clean()["seqs"][2]
    s["pred"] = np.ascontiguousarray(s["pred"][:, :-2, :-4])
    return dict(task="semi-supervised", seqs=[s], error=AssertionError)


def scene_err_unsup_single_metric():
    s = scene_unsup_clean()["seqs"][1]
    return dict(task="unsupervised", seqs=[s], metrics=("J",), error=NameError)


SCENES = {"semi_clean": scene_semi_clean, "semi_fewer_results": scene_semi_fewer_results, "unsup_clean": scene_unsup_clean,
          "unsup_20": scene_unsup_20, "edges": scene_edges, "long_300": scene_long_300, "radius_2": scene_radius_2,
          "err_missing_frame": scene_err_missing_frame, "err_too_many_objects": scene_err_too_many_objects,
          "err_21_proposals": scene_err_21_proposals, "err_size_mismatch": scene_err_size_mismatch,
          "err_unsup_single_metric": scene_err_unsup_single_metric}


def operator_stacks():
    """One pair of 64 x 96 stacks: r = 18 reaches across most of the image and every border."""
    H, W, T = 64, 96, 3
    objs = [(1, 20, 25, 12, 16, 3, 6, 2), (2, 44, 60, 10, 14, -2, 4, 2), (3, 60, 90, 6, 8, 0, 0, 1)]
    gt = paint(T, H, W, objs)
    gt[:, :, 30:33] = 255
    gt[:, 40:42, 50:] = 255
    gt[:, 0, 0:10] = 3
    pred = paint(T, H, W, jitter(objs, 11, 4.0, 3.0) + [(4, 8, 80, 5, 7, 2, -3, 1)])
    pred[:, H - 1, W - 6:] = 4
    pred[2] = np.where(pred[2] == 2, 0, pred[2])                     # result 2 empty in the last frame
    return gt, pred


# ------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------------------
def load_reference():
    """The reference's vos_davis_evaluation module, imported from its file with the stand-ins of the module docstring."""
    import scipy.ndimage
    ref_evaluators()                                                 # detectron2's inert bases, tqdm, the `_ref_evaluation` package
    sys.modules["detectron2.evaluation"].COCOEvaluator = type("COCOEvaluator", (), {})
    if "pycocotools" not in sys.modules:
        pc = types.ModuleType("pycocotools")
        pc.__path__ = []
        pc.mask = types.ModuleType("pycocotools.mask")
        sys.modules["pycocotools"], sys.modules["pycocotools.mask"] = pc, pc.mask
    cv2 = types.ModuleType("cv2")
    cv2.dilate = lambda src, kernel: scipy.ndimage.binary_dilation(src, structure=kernel, border_value=0).astype(np.uint8)
    sk = types.ModuleType("skimage")
    sk.__path__ = []
    sk.morphology = types.ModuleType("skimage.morphology")

    def disk(r):
        a = np.arange(-int(r), int(r) + 1)
        return (a[:, None] ** 2 + a[None, :] ** 2 <= int(r) ** 2).astype(np.uint8)
    sk.morphology.disk = disk
    sys.modules["cv2"], sys.modules["skimage"], sys.modules["skimage.morphology"] = cv2, sk, sk.morphology
    name = "_ref_evaluation.vos_davis_evaluation"
    spec = importlib.util.spec_from_file_location(name, f"{REF_ROOT}/univs/evaluation/vos_davis_evaluation.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def write_tree(root, scene):
    """DAVIS tree + result directory of a scene -> (davis root, res_path).  Shared with tests/davis_eval_cases.py in layout only."""
    resolution = scene.get("resolution", "480p")
    davis, out = os.path.join(root, "DAVIS"), os.path.join(root, "out")
    ann = "Annotations" if scene["task"] == "semi-supervised" else "Annotations_unsupervised"
    os.makedirs(os.path.join(davis, "ImageSets", "2017"), exist_ok=True)
    with open(os.path.join(davis, "ImageSets", "2017", "val.txt"), "w") as f:
        f.write("".join(s["name"] + "\n" for s in scene["seqs"]))
    for s in scene["seqs"]:
        for sub, maps, names in ((os.path.join(davis, ann, resolution, s["name"]), s["gt"], s["gt_names"]),
                                 (os.path.join(out, "Annotations", s["name"]), s["pred"], s["pred_names"])):
            os.makedirs(sub, exist_ok=True)
            for m, n in zip(maps, names):
                Image.fromarray(m).save(os.path.join(sub, n), format="PNG")
        jpg = os.path.join(davis, "JPEGImages", resolution, s["name"])
        os.makedirs(jpg, exist_ok=True)
        for n in s["gt_names"]:
            Image.new("RGB", (8, 8)).save(os.path.join(jpg, n.replace(".png", ".jpg")))
    return davis, out


def run_reference(ref, davis, out, scene):
    """`DAVISEvaluator.evaluate` of the reference -> (returned dictionary, [(j, f) per sequence], text of davis-metrics.txt)."""
    kept = {"res": None, "tables": []}
    ev_davis, semi, unsup = ref.evaluate_davis, ref._evaluate_semisupervised, ref._evaluate_unsupervised

    def keep(fn):
        def wrapped(*a, **k):
            r = fn(*a, **k)
            kept["tables"].append(r)
            return r
        return wrapped

    def keep_res(*a, **k):
        kept["res"] = ev_davis(*a, **k)
        return kept["res"]
    ref.evaluate_davis, ref._evaluate_semisupervised, ref._evaluate_unsupervised = keep_res, keep(semi), keep(unsup)
    try:
        e = object.__new__(ref.DAVISEvaluator)
        e._output_dir, e.task, e.metrics = out, scene["task"], scene.get("metrics", ("J", "F"))
        e.dataset = ref.DAVIS(root=davis, task=scene["task"], subset="val", sequences="all", resolution=scene.get("resolution", "480p"))
        e.evaluate()
    finally:
        ref.evaluate_davis, ref._evaluate_semisupervised, ref._evaluate_unsupervised = ev_davis, semi, unsup
    with open(os.path.join(out, "davis-metrics.txt")) as f:
        return kept["res"], kept["tables"], f.read()


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    ref = load_reference()
    from _ref_evaluation.davis2017_evaluation.davis2017.metrics import db_eval_boundary, db_eval_iou

    gt, pred = operator_stacks()
    G, P = 3, 4
    rec = {"gt": gt, "pred": pred, "G": np.array(G), "P": np.array(P), "radii": np.array(RADII)}
    void = gt == 255
    gm = np.stack([gt == i + 1 for i in range(G)])
    pm = np.stack([pred == j + 1 for j in range(P)])
    for use_void in (0, 1):
        for r in RADII:
            J, F = np.zeros((G, P, len(gt))), np.zeros((G, P, len(gt)))
            for i in range(G):
                for j in range(P):
                    J[i, j] = db_eval_iou(gm[i], pm[j], void if use_void else None)
                    F[i, j] = db_eval_boundary(gm[i], pm[j], void if use_void else None, bound_th=r)
            rec[f"J_v{use_void}_r{r}"], rec[f"F_v{use_void}_r{r}"] = J, F
    path = os.path.join(GOLDEN, "g28_davis_eval_operators.npz")
    np.savez_compressed(path, **rec)
    print("operators", os.path.getsize(path), "bytes")

    for name, make in SCENES.items():
        scene = make()
        error = scene.get("error")
        metrics = scene.get("metrics", ("J", "F"))
        rec = {"task": np.array(scene["task"]), "resolution": np.array(scene.get("resolution", "480p")), "metrics": np.array(metrics),
               "seqs": np.array([s["name"] for s in scene["seqs"]])}
        for s in scene["seqs"]:
            for k in ("gt", "pred"):
                rec[f"{k}_{s['name']}"], rec[f"{k}_names_{s['name']}"] = s[k], np.array(s[k + "_names"])
        with tempfile.TemporaryDirectory() as root:
            davis, out = write_tree(root, scene)
            if error is not None:
                try:
                    run_reference(ref, davis, out, scene)
                except error as e:
                    rec["error"] = np.array(type(e).__name__)
                assert "error" in rec, f"{name}: the reference did not raise"
            else:
                res, tables, text = run_reference(ref, davis, out, scene)
                assert len(tables) == len(scene["seqs"])
                for s, (j, f) in zip(scene["seqs"], tables):
                    rec["j_" + s["name"]], rec["f_" + s["name"]] = np.asarray(j, np.float64), np.asarray(f, np.float64)
                for m in metrics:
                    for k in ("M", "R", "D"):
                        rec[f"{m}_{k}"] = np.array(res[m][k], dtype=np.float64)
                    rec[f"{m}_keys"] = np.array(list(res[m]["M_per_object"].keys()))
                    rec[f"{m}_per_object"] = np.array(list(res[m]["M_per_object"].values()), dtype=np.float64)
                rec["text"] = np.array(text)
        path = os.path.join(GOLDEN, f"g28_davis_eval_{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) <= 66584, f"{name}: {os.path.getsize(path)} bytes"
        print(name, os.path.getsize(path), "bytes", rec.get("error", ""), rec.get("text", ""), sep="\n  ")


if __name__ == "__main__":
    main()
