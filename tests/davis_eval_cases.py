"""What tests/test_davis_eval_cpu.py and tests/test_davis_eval_gpu.py share: the g28 fixtures (tools/gen_golden_davis_eval.py), the
DAVIS trees painted from them, and the comparison of a score with what the reference recorded.  The counts are integers and the scores
the same float64 operations on them: no tolerance anywhere."""
import os

import numpy as np
import torch

from univs_amd.evaluation import davis

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORED = ["semi_clean", "semi_fewer_results", "unsup_clean", "unsup_20", "edges", "long_300", "radius_2"]
ERRORS = ["err_missing_frame", "err_too_many_objects", "err_21_proposals", "err_size_mismatch", "err_unsup_single_metric"]
ERROR_TYPES = {"SystemExit": SystemExit, "AssertionError": AssertionError, "NameError": NameError}
RADII = (1, 2, 5, 8, 18)


def load(name):
    with np.load(os.path.join(GOLDEN, f"g28_davis_eval_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    if "seqs" in fx:
        fx["task"], fx["resolution"] = str(fx["task"]), str(fx["resolution"])
        fx["seqs"], fx["metrics"] = [str(s) for s in fx["seqs"]], tuple(str(m) for m in fx["metrics"])
    return fx


def write_tree(fx, root):
    """The fixture as a DAVIS tree and a result directory: (davis_root, res_path)."""
    from PIL import Image
    root_davis, res = os.path.join(root, "DAVIS"), os.path.join(root, "run", "inference", "Annotations")
    ann = "Annotations" if fx["task"] == "semi-supervised" else "Annotations_unsupervised"
    os.makedirs(os.path.join(root_davis, "ImageSets", "2017"), exist_ok=True)
    with open(os.path.join(root_davis, "ImageSets", "2017", "val.txt"), "w") as f:
        f.write("".join(s + "\n" for s in fx["seqs"]))
    for s in fx["seqs"]:
        for sub, maps, names in ((os.path.join(root_davis, ann, fx["resolution"], s), fx["gt_" + s], fx["gt_names_" + s]),
                                 (os.path.join(res, s), fx["pred_" + s], fx["pred_names_" + s])):
            os.makedirs(sub, exist_ok=True)
            for m, n in zip(maps, names.tolist()):
                Image.fromarray(m).save(os.path.join(sub, n), format="PNG")
        jpg = os.path.join(root_davis, "JPEGImages", fx["resolution"], s)
        os.makedirs(jpg, exist_ok=True)
        for n in fx["gt_names_" + s].tolist():
            Image.new("RGB", (8, 8)).save(os.path.join(jpg, n.replace(".png", ".jpg")))
    return root_davis, res


def same(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True)


def check_tables(fx, device):
    """`sequence_tables` of every sequence straight from the fixture's arrays against the recorded per-frame J / F tables."""
    for s in fx["seqs"]:
        gt, pred = fx["gt_" + s], fx["pred_" + s]
        if fx["task"] == "semi-supervised":
            pred = pred[1:-1]
        j, f = davis.sequence_tables(gt, pred, fx["task"], fx["metrics"], device)
        print(s, "J", j.shape, "F", f.shape, "nan", int(np.isnan(fx["f_" + s]).sum()))
        assert same(j, fx["j_" + s]), s
        assert same(f, fx["f_" + s]), s


def check_result(fx, res, text=None):
    """The dictionary `evaluate_davis_files` returns against the reference's (NaNs in the same places), the text byte for byte."""
    assert list(res) == list(fx["metrics"])
    for m in fx["metrics"]:
        for k in ("M", "R", "D"):
            assert same(res[m][k], fx[f"{m}_{k}"]), (m, k, res[m][k], fx[f"{m}_{k}"])
        assert list(res[m]["M_per_object"]) == fx[f"{m}_keys"].tolist()
        assert same(list(res[m]["M_per_object"].values()), fx[f"{m}_per_object"]), m
    assert davis.metrics_text(res) == str(fx["text"])
    if text is not None:
        assert text == str(fx["text"])


def operator_counts(fx, counts_fn, device):
    """{(use_void, r): (region, n_gt, n_fg, match)} of the operator fixture's stacks from `counts_fn` on `device`."""
    g, p = torch.from_numpy(fx["gt"]).to(device), torch.from_numpy(fx["pred"]).to(device)
    return {(v, r): counts_fn(g, p, int(fx["G"]), int(fx["P"]), r, v) for v in (0, 1) for r in RADII}


def check_operators(fx, counts):
    for (v, r), c in counts.items():
        J, F = davis.jf_from_counts(*c)
        assert same(J, fx[f"J_v{v}_r{r}"]), (v, r)
        assert same(F, fx[f"F_v{v}_r{r}"]), (v, r)


# ---- synthetic inputs of the kernel tests -------------------------------------------------------------------------------------------
def maps(T, H, W, G, P, seed):
    """gt / pred uint8 [T, H, W]: rectangles of every id 1..G / 1..P scattered over the plane, objects on all four borders and the
    bottom-right pixel, void stripes, id 1 missing from the result of frame 0, a last frame without gt objects, a frame that is empty
    on both sides (T > 2), and values beyond the counts, which are background (254 in the gt, 255 in the result)."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((T, H, W), np.uint8)
    pred = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        for m, n, off in ((gt, G, 0), (pred, P, 1)):
            for k in range(1, n + 1):
                h, w = int(rng.integers(1, max(2, H // 3))), int(rng.integers(1, max(2, W // 3)))
                y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
                m[t, min(y + off, H - h):min(y + off, H - h) + h, x:x + w] = k
            m[t, 0, : W // 2] = 1                                     # first row
            m[t, H // 2:, 0] = n                                      # first column
            m[t, H - 1, W // 3:] = 1 + (n > 1)                        # last row, with the bottom-right pixel
            m[t, : H // 3, W - 1] = n                                 # last column
        gt[t, :, W // 2] = 255                                        # void stripes
        gt[t, H // 3, :] = 255
        gt[t, 0, 0] = 254 if G < 254 else 0                           # beyond the counts: background
        if P < 200:
            pred[t, H - 1, 0] = 255
    pred[0][pred[0] == 1] = 0                                         # id 1 on the gt side only
    if T > 1:
        gt[T - 1] = 0                                                 # an empty frame on the gt side
        pred[T - 1, :, : W // 2] = 0
    if T > 2:
        gt[1], pred[1] = np.where(gt[1] == 255, 255, 0), 0            # a frame that is empty on both sides
    return gt, pred
