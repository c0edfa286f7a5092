"""What tests/test_vss_eval_cpu.py and tests/test_vss_eval_gpu.py share: the g27 fixtures (tools/gen_golden_vss_eval.py), the VSPW trees
painted from them, and the comparison of a score with what the reference recorded.  Everything is an integer or a text: no tolerance."""
import os

import numpy as np
import torch

from univs_amd.evaluation import vss

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORED = ["clean", "void_alias", "pred_alias", "short", "one_short_of_16", "all_changing", "dotfiles"]
ERRORS = ["err_overflow", "err_size_mismatch", "err_missing_pred"]
ERROR_TYPES = {"ValueError": ValueError, "AssertionError": AssertionError, "FileNotFoundError": FileNotFoundError}
NUM_CLASSES = 124                                        # fixed by the reference's scripts


def load(name):
    with np.load(os.path.join(GOLDEN, f"g27_vss_eval_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    fx["split"], fx["split_file"] = str(fx["split"]), str(fx["split_file"])
    fx["videos"] = [str(v) for v in fx["videos"]]
    return fx


def write_tree(fx, root, predictions=True):
    """The fixture as a VSPW tree: (submit_dir, data_dir)."""
    from PIL import Image
    data, submit = os.path.join(root, "VSPW"), os.path.join(root, "run", "submit")
    os.makedirs(submit, exist_ok=True)
    for v in fx["videos"]:
        sides = [(os.path.join(data, "data", v, "mask"), fx["gt_" + v], fx["names_" + v])]
        if predictions:
            sides.append((os.path.join(submit, v), fx["pred_" + v], fx["pred_names_" + v]))
        for sub, maps, names in sides:
            os.makedirs(sub, exist_ok=True)
            for m, n in zip(maps, names.tolist()):
                Image.fromarray(m).save(os.path.join(sub, n), format="PNG")
    with open(os.path.join(data, fx["split_file"]), "w") as f:
        f.write(fx["split"])
    return submit, data


def video_counts(fx, device):
    """VideoCounts of every video straight from the fixture's arrays, in split order."""
    out = []
    for v in fx["videos"]:
        names = fx["names_" + v].tolist()
        frames = [(n, g, p) for n, g, p in zip(names, fx["gt_" + v], fx["pred_" + v])]
        out.append(vss.video_counts(v, len(names), frames, NUM_CLASSES, device))
    return out


def check_score(fx, score):
    """`score` (vss.score_counts' dict) against the reference's record: the confusion matrix and the per-window ratios equal (NaN
    positions included), the three texts byte-identical."""
    assert np.array_equal(score["confusion"], fx["confusion"])
    for n in (8, 16):
        got, ref = np.asarray(score["ratios"][n], dtype=np.float64), fx["ratios%d" % n]
        print(f"VC{n}: {len(got)} windows, {int(np.isnan(ref).sum())} nan")
        assert got.shape == ref.shape and np.array_equal(got, ref, equal_nan=True), n
    assert sorted(score["files"]) == fx["file_names"].tolist()
    for name, text in zip(fx["file_names"].tolist(), fx["file_texts"].tolist()):
        assert score["files"][name] == text, (name, score["files"][name], text)


def check_files(fx, directory):
    for name, text in zip(fx["file_names"].tolist(), fx["file_texts"].tolist()):
        with open(os.path.join(directory, name)) as f:
            assert f.read() == text, name


# the evaluator's side: contiguous ids 0..123 of dataset ids 1..124, the ignore value 255
CONTIGUOUS_TO_DATASET = {i: i + 1 for i in range(NUM_CLASSES)}


def vss_outputs(fx, v, device="cpu"):
    """One video of the fixture as `vss_output_results` hands it to `VSSEvaluator.process`: the prediction bytes are contiguous class
    ids already (dataset id - 1), 255 the ignore value."""
    names = fx["pred_names_" + v].tolist()
    pred = fx["pred_" + v]
    inputs = {"video_id": v, "file_names": [f"data/{v}/origin/{n.replace('.png', '.jpg')}" for n in names],
              "frame_indices": list(range(len(names)))}
    outputs = {"image_size": pred.shape[1:], "pred_masks": torch.from_numpy(pred.astype(np.int64)).to(device)}
    return inputs, outputs


# `dotfiles` cannot go through `process`: `write_vss_predictions` names a frame by the text before its first dot, so `.x.jpg` is
# written as `.png` (the reference's evaluator does the same) and the `.x.png` that the mask directory lists has no prediction
EVALUATOR_SCORED = [n for n in SCORED if n != "dotfiles"]


def run_evaluator(fx, root, device, monkeypatch=None):
    """reset / process every video / evaluate on a tree without predictions -> (score, output_dir, data_dir, the paths opened by
    evaluate())."""
    submit, data = write_tree(fx, os.path.join(root, "tree"), predictions=False)
    ev = vss.VSSEvaluator(CONTIGUOUS_TO_DATASET, 255, NUM_CLASSES, data, fx["split_file"], submit, device=device)
    ev.reset()
    for v in fx["videos"]:
        inputs, outputs = vss_outputs(fx, v, device)
        ev.process([inputs], outputs)
    opened = []
    if monkeypatch is not None:
        from PIL import Image
        real = Image.open

        def recording_open(fp, *a, **k):
            opened.append(str(fp))
            return real(fp, *a, **k)
        monkeypatch.setattr(Image, "open", recording_open)
    try:
        score = ev.evaluate()
    finally:
        if monkeypatch is not None:
            monkeypatch.undo()
    return score, submit, data, opened
