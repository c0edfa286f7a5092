"""Mask IoU, boundary IoU and their decay of a VIPOSeg panoptic-VOS result, from one count per video (pvos_counts.py) instead of two
planes eroded d times per (tracked object, frame).

The reference scores the indexed PNGs that its VOS driver writes with `PVOSEvaluator` / `eval_iou`
(univs/evaluation/pvos_evaluation.py:25-264; the stand-alone univs/evaluation/eval_pvos.py is the same loop behind a command line)
over `boundary_iou` (univs/evaluation/eval_utils_viposeg.py:27-80).  Both scores are ratios of exact integer counts, which `pvos_counts`
takes from the two uint8 stacks of a video in one launch for every id; the rest is host arithmetic in float64 with the reference's own
expressions on the same integers and in its order (videos sorted, frames sorted and paired by index, objects in the order they
entered), so `np.mean` sums the same sequences and the numbers and the result text come out the same.

  eval_iou               the reference's function of the same name on the three sorted directory lists
  evaluate_pvos_files    the file-level entry point, the `__main__` of eval_pvos.py: returns the dictionary
  PVOSEvaluator          reset / process / evaluate with the reference's call pattern; writes pvos-ious.txt

Reproduced on purpose: with fewer results than references only the reference list is filtered, the ground-truth list is paired by
index as it stands; an unequal frame count is an AssertionError; an object enters from a reference frame
(`Annotations/<video>/<frame>.png`, its non-zero ids) and is scored from the NEXT frame on; an id that two reference frames name is
tracked, scored and counted twice; an object empty on both sides scores 1 / 1, on one side 0 / 0; class 98 goes by the video's name,
every other class through the four lists in the reference's order, a class in none of them feeds only the decay; an id without an
entry in obj_class.json is a KeyError, and so is the 80th tracked object with the decay on; a group without objects has a NaN mean;
the decay is fitted over fewer than 60 tracked objects; pvos-ious.txt has no line ends and 100 x on the keys that contain 'iou'.

One difference: a frame whose annotation and result differ in size raises ValueError whenever the video tracks an object at that
frame.  The reference raises the same type, but only once an object is non-empty on both sides there.

`python -m univs_amd.evaluation.pvos --res_path ... --data_path ... [--eval_decay] [--reader host|gpu]` scores a result directory.  Single process.
"""
import argparse
import json
import logging
import os
import warnings
from glob import glob

import numpy as np
import torch

from ._counts import check_reader, device_stack, pick_device as _device, stack as _stack
from .pvos_counts import dilation, pvos_counts

# The class partition of VIPOSeg and the videos whose class 98 ("other machine") is unseen: facts of the dataset
# (eval_utils_viposeg.py:5-25; tests/golden/g30_pvos_eval_classes.npz records the reference's lists).
THING_SEEN_CLASS = (60, 89, 90, 8, 48, 2, 79, 106, 76, 84, 114, 74, 108, 91, 83, 85, 54, 65, 78, 44, 92, 122, 107, 43, 88, 117, 50, 51, 87,
                    52, 62, 115, 10, 41, 77, 82, 56, 123, 49, 4, 63)
THING_UNSEEN_CLASS = (102, 99, 109, 47, 55, 61, 118, 72, 46, 96, 64, 101, 86, 97, 100, 116, 95)
STUFF_SEEN_CLASS = (28, 66, 0, 14, 15, 13, 7, 12, 22, 68, 1, 59, 27, 75, 40, 29, 18, 21, 19, 39, 30, 11, 53, 111, 45, 35, 98, 36, 119, 42,
                    104, 23, 80, 93, 67, 3, 31, 16, 69, 103, 37, 121, 110, 105, 33, 24, 70, 73, 32)
STUFF_UNSEEN_CLASS = (9, 71, 120, 58, 94, 5, 34, 20, 6, 26, 112, 17, 57, 113, 25, 81, 38)
OTHER_MACHINE_CLASS = 98
OTHER_MACHINE_VIDEOS = ("187_WUZUSD4477I", "319_l1Dz12fxQzQ", "320_nhKXemkIvh4", "517_AWvYuplla_s", "532_QmZyJuLlEec", "774_devdFjIpDcc",
                        "1016_HG0AsTOxI5g", "1017_IAU0WGB9VPw", "1020_TgCIv6bp3XM", "1021_cPOxAMo28yk", "1022_emSaDd2ddj0",
                        "1033_sh81AwYuihg", "1065_d2sHRyAHKqI", "1067_fk3jhxBi1pA", "1068_gxnZkf0LQfk", "1069_jFHRbZxswz8",
                        "1070_uTJB31tuYes", "1072_zvNEdUk5k0Q", "1230_AGY-gQ_3O8Y", "1333__iprMPKLdOQ", "1334_qlmfvYA3_rk",
                        "2004_1btxeVbyojs", "2005_83KrhWajwfw")
GROUPS = ("thing_seen", "thing_unseen", "stuff_seen", "stuff_unseen")
MAX_TRACKED = 80          # the decay's table has the keys 0 .. 79
DECAY_BELOW = 60          # ... of which the fit takes those below 60


def group_of(class_id, video_id):
    """The group an object of `class_id` in `video_id` is averaged in, or None (pvos_evaluation.py:203-222)."""
    if class_id == OTHER_MACHINE_CLASS:
        return "stuff_unseen" if video_id in OTHER_MACHINE_VIDEOS else "stuff_seen"
    if class_id in THING_UNSEEN_CLASS:
        return "thing_unseen"
    if class_id in STUFF_UNSEEN_CLASS:
        return "stuff_unseen"
    if class_id in THING_SEEN_CLASS:
        return "thing_seen"
    if class_id in STUFF_SEEN_CLASS:
        return "stuff_seen"
    return None


def _read_u8(path):
    from PIL import Image
    with Image.open(path) as im:
        a = np.array(im, np.uint8)
    if a.ndim != 2:
        raise ValueError(f"{path}: {a.shape} is no id map")
    return a


def _read_ids(path):
    from PIL import Image
    with Image.open(path) as im:
        return [x for x in np.unique(np.asarray(im)) if x != 0]


def ious_from_counts(c):
    """(miou, biou) of one object in one frame from its six counts (I, A_g, A_p, BI, B_g, B_p), with the reference's special cases
    (pvos_evaluation.py:190-201, eval_utils_viposeg.py:74-80)."""
    I, Ag, Ap, BI, Bg, Bp = (np.int64(v) for v in c)
    if Ap == 0 and Ag != 0:
        return 0., 0.
    if Ap != 0 and Ag == 0:
        return 0., 0.
    if Ap == 0 and Ag == 0:
        return 1., 1.
    union = Bg + Bp - BI
    return I / (Ag + Ap - I), (0 if union == 0 else BI / union)


def video_counts(labels, preds, tracked, device=None):
    """{frame index: int64 [K, 6]} for the frames of one video at which an object is tracked.  labels / preds: the uint8 maps per
    frame, tracked: the ids tracked per frame.  The frames of one size go up in one stack and through one `pvos_counts` call (a VIPOSeg
    video has one size); ValueError where the two maps of such a frame differ in size."""
    groups = {}
    for i, ids in enumerate(tracked):
        if not ids:
            continue
        if labels[i].shape != preds[i].shape:
            raise ValueError(f"frame {i}: annotation {labels[i].shape} and result {preds[i].shape} differ in size")
        groups.setdefault(labels[i].shape, []).append(i)
    out = {}
    device = _device(device)
    for (H, W), frames in groups.items():
        K = max((int(x) for i in frames for x in tracked[i] if int(x) <= 255), default=0)
        if K == 0:
            continue
        gt = torch.as_tensor(_stack([labels[i] for i in frames])).to(device)
        pr = torch.as_tensor(_stack([preds[i] for i in frames])).to(device)
        counts = pvos_counts(gt, pr, dilation(H, W), K).cpu().numpy().astype(np.int64)
        for n, i in enumerate(frames):
            out[i] = counts[n]
    return out


def eval_iou(res_list, seq_list, ref_list, obj_class_dict, eval_decay=False, device=None, details=None, reader="host"):
    """The reference's `eval_iou`: the dictionary of the eight group means, their four averages, `overall_iou` and, with `eval_decay`,
    `decay`.  `details`, a dictionary, receives the per-object values behind them in the order of scoring: "<group>_miou" and
    "<group>_biou" (lists), "decay" ({tracked objects: [(miou + biou) / 2]}) and "objects" ([(video, frame index, id)]).
    reader "gpu": a video's ground truth and results are decoded on the device (`_counts.device_stack`), one call per side."""
    check_reader(reader)
    miou_lists = {g: [] for g in GROUPS}
    biou_lists = {g: [] for g in GROUPS}
    iou_decay_dict = {i: [] for i in range(MAX_TRACKED)} if eval_decay else {}
    objects = []
    if details is not None:
        details.update({f"{g}_miou": miou_lists[g] for g in GROUPS}, **{f"{g}_biou": biou_lists[g] for g in GROUPS}, decay=iou_decay_dict,
                       objects=objects)
    for s, r, f in zip(seq_list, res_list, ref_list):
        video_id = s.split("/")[-1]
        label_list = sorted(glob(s + "/*"))
        pred_list = sorted(glob(r + "/*"))
        ann_list = sorted(glob(f + "/*"))
        ann_name_list = [x.split("/")[-1] for x in ann_list]
        assert len(label_list) == len(pred_list), "incomplete label/pred"
        labels, preds = device_stack(label_list, reader, device), device_stack(pred_list, reader, device)
        if labels is None or preds is None or labels.shape[1:] != preds.shape[1:]:
            labels = [_read_u8(p) for p in label_list]
            preds = [_read_u8(p) for p in pred_list]
        obj_ids, tracked = [], []
        for i in range(len(label_list)):
            tracked.append(list(obj_ids))
            # exclude obj in ref frames, eval in next frame
            frame_name = label_list[i].split("/")[-1]
            if frame_name in ann_name_list:
                obj_ids.extend(_read_ids(ann_list[ann_name_list.index(frame_name)]))
        counts = video_counts(labels, preds, tracked, device)
        for i, ids in enumerate(tracked):
            obj_num = len(ids)
            for id in ids:
                k = int(id)
                miou, biou = ious_from_counts(counts[i][k - 1] if k <= 255 else (0,) * 6)
                objects.append((video_id, i, k))
                group = group_of(int(obj_class_dict[video_id][str(id)]), video_id)
                if group is not None:
                    miou_lists[group].append(miou)
                    biou_lists[group].append(biou)
                if eval_decay:
                    iou_decay_dict[obj_num].append((miou + biou) / 2.)
    res_dict = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)     # the mean of an empty group is NaN
        for g in GROUPS:
            res_dict[f"{g}_miou"] = np.mean(miou_lists[g])
        for g in GROUPS:
            res_dict[f"{g}_biou"] = np.mean(biou_lists[g])
    for g in GROUPS:
        res_dict[f"{g}_iou"] = (res_dict[f"{g}_miou"] + res_dict[f"{g}_biou"]) / 2
    res_dict["overall_iou"] = (res_dict["thing_seen_iou"] + res_dict["thing_unseen_iou"]
                               + res_dict["stuff_seen_iou"] + res_dict["stuff_unseen_iou"]) / 4
    if eval_decay:
        x, y = [], []
        for k, v in iou_decay_dict.items():
            if v != [] and k < DECAY_BELOW:
                x.append(k)
                y.append(np.mean(v))
        _x = np.expand_dims(np.array(x), -1)
        _y = np.expand_dims(np.array(y), -1)
        A = _x / 100
        b = -np.log(_y)
        decay = np.dot(np.dot(np.linalg.inv(np.dot(A.T, A)), A.T), b)
        res_dict["decay"] = decay[0, 0]
    return res_dict


def _lists(res_path, data_path):
    """(res_list, seq_list, ref_list, obj_class_dict) as the reference collects them (eval_pvos.py:143-159)."""
    res_list = sorted(glob(res_path + "/*"))
    seq_list = sorted(glob(os.path.join(data_path, "Annotations_gt") + "/*"))
    ref_list = sorted(glob(os.path.join(data_path, "Annotations") + "/*"))
    if len(res_list) < len(ref_list):
        res_seqs = [seq_name.split("/")[-1] for seq_name in res_list]
        ref_list = [seq_name for seq_name in ref_list if seq_name.split("/")[-1] in res_seqs]
    assert len(res_list) > 0 and len(res_list) == len(ref_list), "{} results and {} data".format(len(res_list), len(ref_list))
    with open(os.path.join(data_path, "obj_class.json"), "r") as f:
        obj_class_dict = json.load(f)
    return res_list, seq_list, ref_list, obj_class_dict


def evaluate_pvos_files(res_path, data_path, eval_decay=False, device=None, details=None, reader="host"):
    """The scores of the result directory `<res_path>/<video>/<frame>.png` against the VIPOSeg split `data_path` (Annotations_gt,
    Annotations, obj_class.json): the reference's dictionary.  Every PNG is read once; a video's two stacks are uploaded once to
    `device` (default: the GPU when there is one, else the ATen counts on the CPU).  reader "gpu": the id maps are decoded on the
    device instead of by Pillow (the reference frames' ids stay with Pillow: a few files per video).

    Errors as the reference's: AssertionError for no result, for a result count that the references do not match, and for a video with
    unequal frame counts; KeyError for an id without a class and for 80 tracked objects with the decay on; ValueError for a frame
    whose two maps differ in size while an object is tracked (module docstring)."""
    return eval_iou(*_lists(res_path, data_path), eval_decay, device, details, reader)


def scores_text(res_dict):
    """The text of pvos-ious.txt (pvos_evaluation.py:132-138): no line ends, 100 x on the keys that contain 'iou'."""
    return "".join(f"{k} : {res_dict[k] * 100 if 'iou' in k else res_dict[k]}" for k in res_dict)


class PVOSEvaluator:
    """The reference's `PVOSEvaluator` (pvos_evaluation.py:25-138) with the dataset's `image_root` as an explicit argument in place of
    detectron2's MetadataCatalog: the split is `image_root` minus its last component.  `process` is empty, as in the reference: the
    driver has already written the PNGs to `<output_dir>/Annotations`."""

    def __init__(self, dataset_name, image_root, tasks=None, distributed=True, output_dir=None, device=None, reader="host"):
        self._logger = logging.getLogger(__name__)
        self.dataset_name, self._tasks, self._distributed, self._output_dir, self.device = dataset_name, tasks, distributed, output_dir, device
        self.data_path = "/".join(image_root.split("/")[:-1])
        self.eval_decay = True
        self.reader = check_reader(reader)                           # ("host" | "gpu": who decodes the PNGs, _counts.device_stack)

    def reset(self):
        os.makedirs(os.path.join(self._output_dir, "Annotations"), exist_ok=True)

    def process(self, inputs, outputs):
        """Nothing: the VOS driver writes the PNGs itself."""

    def evaluate(self):
        """`eval_iou` on `<output_dir>/Annotations` with the decay; pvos-ious.txt into `output_dir`.  Returns the dictionary (the
        reference returns nothing)."""
        res_dict = evaluate_pvos_files(os.path.join(self._output_dir, "Annotations"), self.data_path, self.eval_decay, self.device,
                                       reader=self.reader)
        self._logger.info("Evaluation results for {}: \n".format(self.dataset_name))
        with open(os.path.join(self._output_dir, "pvos-ious.txt"), "w") as fh:
            fh.write(scores_text(res_dict))
        for k in res_dict:
            v = res_dict[k] * 100 if "iou" in k else res_dict[k]
            print("{}: {:.2f}".format(k, v))
            self._logger.info("{}: {:.2f}".format(k, v))
        return res_dict


def main(argv=None):
    ap = argparse.ArgumentParser(description="mask IoU, boundary IoU and decay of a VIPOSeg panoptic-VOS result directory")
    ap.add_argument("--data_path", type=str, default="./VIPOSeg/valid", help="the split: Annotations_gt, Annotations, obj_class.json")
    ap.add_argument("--res_path", type=str, required=True, help="the result directory: <video>/<frame>.png")
    ap.add_argument("--eval_decay", action="store_true")
    ap.add_argument("--device", default=None, help="cuda / cpu (default: the GPU when there is one)")
    ap.add_argument("--reader", default="host", choices=("host", "gpu"), help="who decodes the PNGs: Pillow on the host, or the device")
    a = ap.parse_args(argv)
    res_dict = evaluate_pvos_files(a.res_path, a.data_path, a.eval_decay, a.device, reader=a.reader)
    for k in res_dict:
        print("{}: {:.2f}".format(k, res_dict[k] * 100 if "iou" in k else res_dict[k]))
    return res_dict


if __name__ == "__main__":
    main()
