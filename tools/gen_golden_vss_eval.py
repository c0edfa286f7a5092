"""Golden fixtures of the VSS scoring (tests/golden/g27_vss_eval_*.npz): the reference's own scripts `eval_miou_vss.py` and
`eval_vc_perclip_vss.py` (univs/evaluation/) run on small synthetic VSPW trees in a temporary directory.

Both scripts run from their own directory (`eval_miou_vss.py` imports `eval_utils_vss` by bare name) with their command line in
`sys.argv`.  `Evaluator.add_batch` is wrapped to keep the evaluator, whose confusion matrix is read at the end, and the VC script's
`get_common` is wrapped to keep the per-window ratios; nothing else of the reference runs differently.  The scripts fix 124 classes.

Each fixture holds the raw uint8 maps of every video of the tree (`gt_<video>`, `pred_<video>` with their file names), the split text
and, for a scene the reference scores: the confusion matrix, the text of the three result files and the ratio list of each clip length.
An error scene holds the exception's type name instead.

Scenes: `clean` (videos of 20, 17 and 9 frames, moving regions, flickering predictions); `void_alias` (pixels that alternate between raw
0 and raw 255: one label after the map; raw values 125..254: outside mIoU, inside VC); `pred_alias` (predictions of 255 that the
flattened confusion matrix counts in a later row); `short` (no video longer than 8 frames: both VC scores are nan); `one_short_of_16`
(16 frames: VC16 skips the video, VC8 scores 8 windows); `all_changing` (a video whose ground truth changes everywhere, every ratio
nan, beside a normal one); `dotfiles` (a `.hidden` line of the split and `.x.png` files in mask directories: counted by mIoU, left out
by VC); and the error scenes `err_overflow`, `err_size_mismatch`, `err_missing_pred`.

    python tools/gen_golden_vss_eval.py     # needs the reference tree (dev container only)
"""
import importlib.util
import os
import runpy
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
from oracle.ref_harness import REF_ROOT                 # noqa: E402  (UNIVS_REFERENCE_ROOT)

REF_EVAL = os.path.join(REF_ROOT, "univs", "evaluation")
H, W = 48, 80
SPLIT_FILE = "val.txt"


def street(T, seed, h=H, w=W, noise=0.01):
    """Raw gt: three bands (raw 5, 17, 124), a rectangle of raw 60 moving right, a static void corner (255) and a static "others" patch
    (0).  Prediction: the mapped gt with the rectangle one pixel off, a patch that flickers every third frame and single-pixel noise."""
    rng = np.random.default_rng(seed)
    gt = np.zeros((T, h, w), np.uint8)
    pred = np.zeros((T, h, w), np.uint8)
    for t in range(T):
        for m, off in ((gt, 0), (pred, 1)):
            m[t, :h // 3], m[t, h // 3:2 * h // 3], m[t, 2 * h // 3:] = 5, 17, 124
            x0 = min(w - 20, 5 + 2 * t + off)
            m[t, 10 + off:25 + off, x0:x0 + 18] = 60
        gt[t, :8, w - 10:] = 255
        gt[t, h - 6:, :12] = 0
    pred -= 1                                                         # raw -> class ids (no 0 among them)
    for t in range(T):
        if t % 3 == 0:
            pred[t, 30:36, 40:50] = 20
        flip = rng.random((h, w)) < noise
        pred[t][flip] = rng.integers(0, 124, int(flip.sum()))
    return gt, pred


def video(vid, gt, pred, names=None, pred_names=None):
    names = names or ["%08d.png" % (t + 1) for t in range(len(gt))]
    return {"video": vid, "names": names, "gt": gt, "pred": pred, "pred_names": pred_names or names}


def scene_clean():
    return [video("v_a", *street(20, 1)), video("v_b", *street(17, 2)), video("v_c", *street(9, 3))], None


def scene_void_alias():
    gt, pred = street(12, 4)
    for t in range(12):
        gt[t, 20:40, 50:70] = 0 if t % 2 else 255                     # one label after the map: common in every window
        gt[t, 40:46, 20:60] = (130, 200, 254)[t // 5]                 # mapped 129 / 199 / 253: not below 124
    gt[:, 0:4, 0:30] = 125                                            # mapped 124: the first value outside
    return [video("v_alias", gt, pred), video("v_d", *street(10, 5))], None


def scene_pred_alias():
    gt, pred = street(11, 6)
    pred[:, 0:10, 0:40] = 255                                         # on raw 5 (mapped 4): cell 124 * 4 + 255, row 6
    pred[3:, 20:30, 60:80] = 255                                      # on raw 17 and 60
    assert (124 * (gt[pred == 255].astype(int) - 1) + 255).max() < 124 * 124 and (gt[pred == 255] > 0).all()
    return [video("v_p", gt, pred)], None


def scene_short():
    return [video("v_8", *street(8, 7)), video("v_5", *street(5, 8))], None


def scene_one_short_of_16():
    return [video("v_16", *street(16, 9))], None


def scene_all_changing():
    gt, pred = street(12, 10)
    for t in range(12):
        gt[t] = 1 + (gt[t].astype(int) + 7 * t) % 120                 # another value at every pixel in every frame
    return [video("v_change", gt, pred), video("v_e", *street(10, 11))], None


def scene_dotfiles():
    ga, pa = street(9, 12)
    gb, pb = street(13, 13)
    gh, ph = street(10, 14)
    names_a = ["%08d.png" % (t + 1) for t in range(8)] + [".x.png"]    # 9 entries pass the length test; 8 frames give no window
    names_b = ["%08d.png" % (t + 1) for t in range(5)] + [".x.png"] + ["%08d.png" % (t + 1) for t in range(5, 12)]
    return [video("v_a", ga, pa, names_a), video(".hidden", gh, ph), video("v_b", gb, pb, names_b)], None


def scene_err_overflow():
    gt, pred = street(4, 15)
    pred[2, 40:44, 30:40] = 255                                       # on raw 124 (mapped 123): cell 124 * 123 + 255 >= 124^2
    return [video("v_o", gt, pred)], ValueError


def scene_err_size_mismatch():
    gt, _ = street(4, 16)
    _, pred = street(4, 16, h=H - 2, w=W - 4)
    return [video("v_s", gt, pred)], AssertionError


def scene_err_missing_pred():
    gt, pred = street(10, 17)
    names = ["%08d.png" % (t + 1) for t in range(10)]
    return [video("v_m", gt, pred[:9], names, names[:9])], FileNotFoundError


SCENES = {"clean": scene_clean, "void_alias": scene_void_alias, "pred_alias": scene_pred_alias, "short": scene_short,
          "one_short_of_16": scene_one_short_of_16, "all_changing": scene_all_changing, "dotfiles": scene_dotfiles,
          "err_overflow": scene_err_overflow, "err_size_mismatch": scene_err_size_mismatch, "err_missing_pred": scene_err_missing_pred}


def write_tree(root, videos):
    data, submit = os.path.join(root, "VSPW"), os.path.join(root, "submit")
    for v in videos:
        for sub, maps, names in ((os.path.join(data, "data", v["video"], "mask"), v["gt"], v["names"]),
                                 (os.path.join(submit, v["video"]), v["pred"], v["pred_names"])):
            os.makedirs(sub, exist_ok=True)
            for m, n in zip(maps, names):
                Image.fromarray(m).save(os.path.join(sub, n), format="PNG")
    split = "".join(v["video"] + "\n" for v in videos)
    with open(os.path.join(data, SPLIT_FILE), "w") as f:
        f.write(split)
    return data, submit, split


def run_reference(data, submit):
    """The two scripts as their command lines run them -> (confusion matrix, {clip length: ratios})."""
    kept = {"evaluator": None, "ratios": {8: [], 16: []}}
    argv, cwd, path = sys.argv, os.getcwd(), list(sys.path)
    os.chdir(REF_EVAL)
    sys.path.insert(0, REF_EVAL)
    try:
        import eval_utils_vss
        add_batch = eval_utils_vss.Evaluator.add_batch

        def keep_evaluator(self, gt_image, pre_image):
            kept["evaluator"] = self
            return add_batch(self, gt_image, pre_image)
        eval_utils_vss.Evaluator.add_batch = keep_evaluator
        sys.argv = ["eval", "--submit_dir", submit, "--data_dir", data, "--split_file", SPLIT_FILE]
        try:
            runpy.run_path(os.path.join(REF_EVAL, "eval_miou_vss.py"), run_name="__main__")
        finally:
            eval_utils_vss.Evaluator.add_batch = add_batch
        spec = importlib.util.spec_from_file_location("eval_vc_perclip_vss", os.path.join(REF_EVAL, "eval_vc_perclip_vss.py"))
        vc = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(vc)
        get_common = vc.get_common

        def keep_ratios(imglist, predlist, clip_num, h, w):
            accs = get_common(imglist, predlist, clip_num, h, w)
            kept["ratios"][clip_num].extend(accs)
            return accs
        vc.get_common = keep_ratios
        vc.main()
    finally:
        sys.argv, sys.path[:] = argv, path
        os.chdir(cwd)
    return kept["evaluator"].confusion_matrix, kept["ratios"]


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    for name, make in SCENES.items():
        videos, error = make()
        assert all(v["gt"].shape[0] <= 20 and v["gt"].shape[1] <= 48 and v["gt"].shape[2] <= 80 for v in videos)
        with tempfile.TemporaryDirectory() as root:
            data, submit, split = write_tree(root, videos)
            rec = {"split": np.array(split), "split_file": np.array(SPLIT_FILE), "videos": np.array([v["video"] for v in videos])}
            for v in videos:
                rec["gt_" + v["video"]], rec["pred_" + v["video"]] = v["gt"], v["pred"]
                rec["names_" + v["video"]], rec["pred_names_" + v["video"]] = np.array(v["names"]), np.array(v["pred_names"])
            if error is not None:
                try:
                    run_reference(data, submit)
                except error as e:
                    rec["error"] = np.array(type(e).__name__)
                assert "error" in rec, f"{name}: the reference did not raise"
            else:
                confusion, ratios = run_reference(data, submit)
                assert (confusion == np.round(confusion)).all()
                rec["confusion"] = confusion.astype(np.int64)
                files = ["miou-final.txt", "vc16-final.txt", "vc8-final.txt"]
                assert sorted(f for f in os.listdir(submit) if f.endswith(".txt")) == files
                rec["file_names"] = np.array(files)
                rec["file_texts"] = np.array([open(os.path.join(submit, f)).read() for f in files])
                for n in (8, 16):
                    rec["ratios%d" % n] = np.array(ratios[n], dtype=np.float64)
        path = os.path.join(GOLDEN, f"g27_vss_eval_{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, os.path.getsize(path), "bytes", rec.get("error", ""), *(rec.get("file_texts", [])), sep="\n  ")


if __name__ == "__main__":
    main()
