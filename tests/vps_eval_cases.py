"""What tests/test_vps_eval_cpu.py and tests/test_vps_eval_gpu.py share: the g26 fixtures (tools/gen_golden_vps_eval.py), the trees
painted from them, and the comparison of a score with what the reference recorded."""
import json
import os

import numpy as np
import torch

from univs_amd.evaluation import vps

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCORED = ["clean", "crowd_void", "enter_leave", "short", "big_tables"]
ERRORS = ["err_png_not_json", "err_json_not_png", "err_area_mismatch", "err_unknown_category", "err_size_mismatch"]
# float64 sums of fewer than 10^3 terms, each <= 1, at 2.2e-16 per reordering: far inside 1e-9 (and equal when the order is kept)
TOL = 1e-9


def load(name):
    with np.load(os.path.join(GOLDEN, f"g26_vps_eval_{name}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    fx["gt_json"], fx["pred_json"] = json.loads(str(fx["gt_json"])), json.loads(str(fx["pred_json"]))
    return fx


def ids_to_rgb(ids):
    return np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], axis=-1).astype(np.uint8)


def write_tree(fx, root):
    """The fixture as a VIPSeg tree: (submit_dir, truth_dir, pan_gt_json_file)."""
    from PIL import Image
    submit, truth = os.path.join(root, "submit"), os.path.join(root, "truth")
    for video in fx["gt_json"]["videos"]:
        vid = video["video_id"]
        for sub, key in ((os.path.join(truth, vid), "gt_" + vid), (os.path.join(submit, "pan_pred", vid), "pred_" + vid)):
            os.makedirs(sub, exist_ok=True)
            for t, im in enumerate(video["images"]):
                Image.fromarray(ids_to_rgb(fx[key][t])).save(os.path.join(sub, im["file_name"]))
    with open(os.path.join(submit, "pred.json"), "w") as f:
        json.dump(fx["pred_json"], f)
    gt_file = os.path.join(root, "gt.json")
    with open(gt_file, "w") as f:
        json.dump(fx["gt_json"], f)
    return submit, truth, gt_file


def tables(fx, device):
    """VideoTables of every video straight from the fixture's arrays: the ground truth as RGB, the prediction as an int32 id map."""
    gt_j, pred_j = vps._by_video(fx["gt_json"]), vps._by_video(fx["pred_json"])
    out = []
    for video in fx["gt_json"]["videos"]:
        vid = video["video_id"]
        gt, pred = fx["gt_" + vid], fx["pred_" + vid]
        assert gt.shape == pred.shape, f"Dismatch shape {gt.shape} and {pred.shape}"
        out.append(vps.video_tables(vid, gt_j[vid], pred_j[vid], ids_to_rgb(gt), pred.astype(np.int32), device))
    return out


def check_score(fx, score):
    """`score` (vps.score_tables' dict) against the reference's record: counts equal, sums within TOL, texts identical."""
    for nframes in vps.NFRAMES:
        r = score["vpq"][nframes]
        cats = [int(c) for c in fx[f"vpq{nframes}_cats"]]
        assert list(r["per_class"]) == cats
        for k in ("tp", "fp", "fn"):
            assert [r["per_class"][c][k] for c in cats] == fx[f"vpq{nframes}_{k}"].tolist(), (nframes, k)
        iou = np.array([r["per_class"][c]["iou"] for c in cats])
        print(f"nframes {nframes}: max |iou - ref| = {np.abs(iou - fx[f'vpq{nframes}_iou']).max():.3e}")
        assert np.abs(iou - fx[f"vpq{nframes}_iou"]).max() <= TOL
        avg = np.array([[r[n]["pq"], r[n]["sq"], r[n]["rq"], r[n]["n"]] for n in ("All", "Things", "Stuff")])
        assert np.abs(avg - fx[f"vpq{nframes}_avg"]).max() <= TOL
    s = score["stq"]
    got = np.array([s["STQ"], s["AQ"], s["IoU"]])
    print(f"STQ / AQ / IoU {got} - ref = {got - fx['stq']}")
    assert np.abs(got - fx["stq"]).max() <= TOL
    for k in ("STQ_per_seq", "AQ_per_seq", "IoU_per_seq", "Length_per_seq"):
        assert np.abs(np.asarray(s[k], dtype=np.float64) - fx[k.lower()]).max() <= TOL, k
    assert sorted(score["files"]) == fx["file_names"].tolist()
    for name, text in zip(fx["file_names"].tolist(), fx["file_texts"].tolist()):
        assert score["files"][name] == text, name


def check_files(fx, directory):
    for name, text in zip(fx["file_names"].tolist(), fx["file_texts"].tolist()):
        with open(os.path.join(directory, name)) as f:
            assert f.read() == text, name


ERROR_TYPES = {"KeyError": KeyError, "AssertionError": AssertionError}


def vps_outputs(fx, vid, device="cpu"):
    """One video of the fixture as `vps_output_results` hands it to `VPSEvaluator.process`: int32 segment ids 1, 2, ... in place of the
    colour ids, with the metadata (1-based category ids, colours) that `write_vps_predictions` expects."""
    pred = fx["pred_" + vid]
    frames = vps._by_video(fx["pred_json"])[vid]
    cat_of = {}
    for fr in frames:
        for el in fr["segments_info"]:
            cat_of.setdefault(int(el["id"]), int(el["category_id"]))
    seg = np.zeros_like(pred, dtype=np.int32)
    infos = []
    for k, (cid, cat) in enumerate(cat_of.items()):
        seg[pred == cid] = k + 1
        infos.append({"id": k + 1, "isthing": bool(fx["gt_json"]["categories"][cat]["isthing"]), "category_id": cat + 1})
    video = next(v for v in fx["gt_json"]["videos"] if v["video_id"] == vid)
    names = [f"frames/{vid}/{im['file_name'].replace('.png', '.jpg')}" for im in video["images"]]
    inputs = {"file_names": names, "frame_indices": list(range(len(names)))}
    outputs = {"image_size": pred.shape[1:], "pred_masks": torch.from_numpy(seg).to(device), "segments_infos": infos}
    return inputs, outputs


def metadata_categories(fx):
    return {c["id"] + 1: {"id": c["id"] + 1, "isthing": c["isthing"], "color": c["color"]} for c in fx["gt_json"]["categories"]}


def run_evaluator(fx, root, device, monkeypatch=None):
    _, truth, gt_file = write_tree(fx, os.path.join(root, "tree"))
    out_dir = os.path.join(root, "out")
    ev = vps.VPSEvaluator(metadata_categories(fx), gt_file, truth, out_dir, device=device)
    ev.reset()
    np.random.seed(0)                                    # (the writer's IdGenerator draws the colours of repeated thing categories)
    for video in fx["gt_json"]["videos"]:
        inputs, outputs = vps_outputs(fx, video["video_id"], device)
        ev.process([inputs], outputs)
    opened = []
    if monkeypatch is not None:
        from PIL import Image
        real = Image.open

        def recording_open(fp, *a, **k):
            opened.append(str(fp))
            return real(fp, *a, **k)
        monkeypatch.setattr(Image, "open", recording_open)
    score = ev.evaluate()
    if monkeypatch is not None:
        monkeypatch.undo()
    return score, out_dir, truth, gt_file, opened
