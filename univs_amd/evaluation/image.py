"""PQ and mIoU of per-image results (inference/image_generic_seg.py): the two evaluators the reference's image configs name
(train_net.py:125-135: `coco_panoptic_seg` / `ade20k_panoptic_seg` -> detectron2's COCOPanopticEvaluator and SemSegEvaluator), with
explicit arguments in place of detectron2's MetadataCatalog and the counts made on the device.

  PanopticEvaluator   reset / process / evaluate.  `process` writes the image's panoptic PNG (results.write_panoptic_prediction) and
                      counts its pair table at once -- `pair_counts` at T = 1 on the int32 prediction against the decoded ground-truth
                      PNG; `evaluate` reads no PNG again.  PQ is `vps.vpq_from_tables` at nframes = 1 (`pq_from_tables`): the reference's own
                      `vpq_compute_single_core(nframes=1)` + `PQStat.pq_average` (univs/evaluation/eval_vpq_vps.py:24-234), which is
                      panopticapi's `pq_compute_single_core` with tubes of one frame: a match is IoU > 0.5, a prediction's VOID overlap
                      is taken out of the union, crowd ground truth is never a false negative, a prediction whose VOID plus same-class
                      crowd overlap exceeds half its area is not a false positive, the ground-truth area is recounted from the PNG.
                      The three KeyErrors of the reference keep their text.  panopticapi and COCOPanopticEvaluator themselves are
                      absent here and stay unpinned.
  SemSegEvaluator     reset / process / evaluate.  `process` adds the image's confusion matrix on the device
                      (imagelabels_ops.label_confusion: csrc/semseg_labels.hip) from `sem_seg_labels` (or the argmax of `sem_seg`);
                      `evaluate` is detectron2's rule (`semseg_scores`), restated from its documented behaviour, unpinned.
  evaluate_panoptic_files / evaluate_semseg_files, and `python -m univs_amd.evaluation.image`: files already on disk.

Mask AP is scored by evaluation/coco.py (COCO's instance ground truth is polygons: polygon_ops.py).  Single process.
"""
import argparse
import json
import os
from collections import OrderedDict

import numpy as np
import torch

from .. import imagelabels_ops
from ._counts import check_reader, device_stack, pick_device, read_png
from .vps import _pq_average, _read_rgb, _vpq_video, video_tables, vpq_text

PQ_KEYS = (("All", ""), ("Things", "_th"), ("Stuff", "_st"))


# ------------------------------------------------------------------------------------------------------------------------------------
# PQ
# ------------------------------------------------------------------------------------------------------------------------------------
def pq_from_tables(images, categories):
    """(the nine numbers x 100, {"All" / "Things" / "Stuff": {"pq", "sq", "rq", "n"}, "per_class": ...}): `vps.vpq_from_tables` at
    nframes = 1, i.e. `_vpq_video` per image and `_pq_average` per group.  `images`: one VideoTables of a single frame per image, in the
    ground truth's order; `categories`: {category id: record}, in the json's order.  One deviation: a group none of whose classes
    occurs (n = 0: a few images without a thing, say) is nan here, where `pq_average` divides by zero."""
    stat = {}
    for v in images:
        _vpq_video(v, categories, 1, stat)
    res = {}
    for name, isthing in (("All", None), ("Things", True), ("Stuff", False)):
        try:
            res[name], per_class = _pq_average(stat, categories, isthing)
        except ZeroDivisionError:
            res[name], per_class = {"pq": float("nan"), "sq": float("nan"), "rq": float("nan"), "n": 0}, None
        if name == "All" and per_class is not None:
            res["per_class"] = per_class
    res.setdefault("per_class", OrderedDict())
    numbers = OrderedDict()
    for name, suffix in PQ_KEYS:
        for k in ("pq", "sq", "rq"):
            numbers[k.upper() + suffix] = 100 * res[name][k]
    return numbers, res


def pq_final_text(numbers):
    return "".join("%s:%.4f\n" % (k, v) for k, v in numbers.items())


def _pred_ids_map(pred):
    """The prediction as pair_counts takes it: an RGB uint8 [H, W, 3] map stays, an id map becomes int32."""
    pred = pred if isinstance(pred, torch.Tensor) else torch.as_tensor(np.asarray(pred))
    return pred if pred.dtype == torch.uint8 and pred.dim() == 3 else pred.to(torch.int32)


class PanopticEvaluator:
    """`pan_gt_json`: the ground truth in COCO's panoptic format ({"images", "annotations": [{"image_id", "file_name",
    "segments_info": [{"id", "category_id", "iscrowd", "area"}]}], "categories"}), `truth_dir` the folder of its PNGs, `output_dir`
    where `inference/panoptic/<stem>.png`, `inference/predictions.json` and `inference/pq-final.txt` go.  `class_table`
    (data.class_table) maps the driver's contiguous classes back to dataset ids; by default it is read from the json's categories."""

    def __init__(self, pan_gt_json, truth_dir, output_dir, class_table=None, device=None, png="host", reader="host"):
        from ..data.image_datasets import class_table as make_table
        with open(pan_gt_json) as f:
            self._gt = json.load(f)
        self.categories = OrderedDict((c["id"], c) for c in self._gt["categories"])
        self.table = class_table if class_table is not None else make_table(self._gt["categories"])
        self._gt_by_image = {str(a["image_id"]): a for a in self._gt["annotations"]}
        self.truth_dir, self._output_dir, self.device, self.png = truth_dir, output_dir, device, png
        self.reader = check_reader(reader)
        self.reset()

    def reset(self):
        self._predictions, self._tables, self.last = [], {}, None

    def _gt_map(self, path, device):
        g = device_stack([path], self.reader, device, rgb=True)
        return g if g is not None else _read_rgb(path)[0][None]

    def count(self, image_id, record, pred_map):
        """The one-frame VideoTables of an image: its ground-truth record and PNG against `record` and the prediction's map."""
        gt = self._gt_by_image.get(str(image_id))
        if gt is None:
            raise KeyError(f"image {image_id!r} has no annotation in the ground truth")
        pred = _pred_ids_map(pred_map)
        device = pick_device(self.device, pred)
        g = self._gt_map(os.path.join(self.truth_dir, gt["file_name"]), device)
        assert tuple(g.shape[1:3]) == tuple(pred.shape[:2]), f"Dismatch shape {tuple(g.shape[1:3])} and {tuple(pred.shape[:2])}"
        return video_tables(str(image_id), [gt], [record], g, pred[None], device)

    def process(self, inputs, outputs):
        from ..inference.results import write_panoptic_prediction
        for item, output in zip(inputs, outputs):
            record = write_panoptic_prediction(item, output, self._output_dir, self.table["ids"], png=self.png)
            self._predictions.append(record)
            self._tables[str(record["image_id"])] = self.count(record["image_id"], record, output["panoptic_seg"][0])

    def evaluate(self):
        if not self._predictions:
            return {}
        save_dir = os.path.join(self._output_dir, "inference")
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, "predictions.json"), "w") as f:
            json.dump({"annotations": self._predictions}, f)
        out, self.last = score_panoptic(self._gt, self._tables, self.categories, save_dir)      # (`last["per_class"]`: tp / fp / fn / iou)
        return out


def score_panoptic(gt_json, tables, categories, save_dir=None):
    """({"panoptic_seg": the nine numbers}, vpq_from_tables' record with its "per_class") of the images' tables in the ground truth's order; an image of the ground truth without a
    prediction is said and left out, as the reference's VPQ script does for a video.  Writes pq-final.txt and pq-per-class.txt."""
    images = []
    for ann in gt_json["annotations"]:
        t = tables.get(str(ann["image_id"]))
        if t is None:
            print(f"{ann['image_id']} does not in prediced json, please double check!!")
            continue
        images.append(t)
    numbers, res = pq_from_tables(images, categories)
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, "pq-final.txt"), "w") as f:
            f.write(pq_final_text(numbers))
        with open(os.path.join(save_dir, "pq-per-class.txt"), "w") as f:
            f.write(vpq_text(res))
    return OrderedDict(panoptic_seg=numbers), res


def evaluate_panoptic_files(panoptic_dir, pan_gt_json, truth_dir, predictions_json=None, device=None, reader="host", output_dir=None):
    """PQ of PNGs already on disk: `panoptic_dir/<file_name>` per record of `predictions_json` (default: `panoptic_dir/../predictions.json`,
    where PanopticEvaluator writes it)."""
    ev = PanopticEvaluator(pan_gt_json, truth_dir, output_dir or os.path.dirname(os.path.normpath(panoptic_dir)), device=device, reader=reader)
    with open(predictions_json or os.path.join(os.path.dirname(os.path.normpath(panoptic_dir)), "predictions.json")) as f:
        records = json.load(f)["annotations"]
    device = pick_device(device)
    for rec in records:
        path = os.path.join(panoptic_dir, rec["file_name"])
        p = device_stack([path], ev.reader, device, rgb=True)
        p = p[0] if p is not None else torch.as_tensor(_read_rgb(path)[0])
        ev._tables[str(rec["image_id"])] = ev.count(rec["image_id"], rec, p)
    return score_panoptic(ev._gt, ev._tables, ev.categories, output_dir)[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# mIoU
# ------------------------------------------------------------------------------------------------------------------------------------
def semseg_scores(conf, class_names=None):
    """detectron2's `SemSegEvaluator.evaluate` on a confusion matrix [(K + 1), (K + 1)] with row = ground truth (row K: ignored pixels,
    left out), column = prediction, in float64: over the K x K block tp = diag, pos_gt = row sums, pos_pred = column sums;
    acc = tp / pos_gt where pos_gt > 0; iou = tp / (pos_gt + pos_pred - tp) where pos_gt > 0 and the union > 0; mIoU and mACC the means
    over those classes, fwIoU = sum(iou pos_gt / sum(pos_gt)) over them, pACC = sum(tp) / sum(pos_gt); a class that is not valid is nan.
    Keys: mIoU, fwIoU, IoU-<name>..., mACC, pACC, ACC-<name>..., each x 100."""
    conf = np.asarray(conf, dtype=np.int64)
    K = conf.shape[0] - 1
    names = [str(n) for n in class_names] if class_names is not None else [str(i) for i in range(K)]
    assert len(names) == K, f"{len(names)} class names for {K} classes"
    block = conf[:K, :K]
    tp = np.diag(block).astype(np.float64)
    pos_gt = block.sum(axis=1).astype(np.float64)
    pos_pred = block.sum(axis=0).astype(np.float64)
    acc = np.full(K, np.nan)
    iou = np.full(K, np.nan)
    acc_valid = pos_gt > 0
    acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
    union = pos_gt + pos_pred - tp
    iou_valid = acc_valid & (union > 0)
    iou[iou_valid] = tp[iou_valid] / union[iou_valid]
    with np.errstate(divide="ignore", invalid="ignore"):
        macc = np.sum(acc[acc_valid]) / np.sum(acc_valid)
        miou = np.sum(iou[iou_valid]) / np.sum(iou_valid)
        class_weights = pos_gt / np.sum(pos_gt)
        fiou = np.sum(iou[iou_valid] * class_weights[iou_valid])
        pacc = np.sum(tp) / np.sum(pos_gt)
    res = OrderedDict()
    res["mIoU"] = 100 * miou
    res["fwIoU"] = 100 * fiou
    for i, name in enumerate(names):
        res["IoU-" + name] = 100 * iou[i]
    res["mACC"] = 100 * macc
    res["pACC"] = 100 * pacc
    for i, name in enumerate(names):
        res["ACC-" + name] = 100 * acc[i]
    return res


class SemSegEvaluator:
    """The ground truth is a folder of class-id PNGs named after the images (`sem_gt_dir/<stem>.png`) or the records' own
    `sem_seg_file_name`; its values are contiguous classes below `num_classes` and `ignore_label`.  `process` uploads (or, reader
    "gpu", decodes on the device) the PNG and adds the image's counts to one int64 matrix there; nothing is read back before
    `evaluate`, which also raises the ValueError of a ground-truth value that is neither."""

    def __init__(self, sem_gt_dir=None, num_classes=None, ignore_label=255, class_names=None, output_dir=None, records=None, device=None,
                 png="host", reader="host"):
        if num_classes is None:
            raise ValueError("SemSegEvaluator: num_classes")
        self.sem_gt_dir, self.num_classes, self.ignore_label = sem_gt_dir, int(num_classes), int(ignore_label)
        self.class_names, self._output_dir, self.device, self.png = class_names, output_dir, device, png
        self._files = {str(r["image_id"]): r["sem_seg_file_name"] for r in (records or []) if "sem_seg_file_name" in r}
        self.reader = check_reader(reader)
        self.reset()

    def reset(self):
        self._conf = self._stray = None
        self._processed = 0

    def gt_path(self, item):
        if "sem_seg_file_name" in item:
            return item["sem_seg_file_name"]
        name = item["file_name"] if "file_name" in item else item["file_names"][0]
        stem = os.path.splitext(os.path.basename(name))[0]
        key = str(item.get("image_id", stem))
        if key in self._files:
            return self._files[key]
        if self.sem_gt_dir is None:
            raise KeyError(f"image {key!r} has no sem_seg_file_name and no sem_gt_dir was given")
        return os.path.join(self.sem_gt_dir, stem + ".png")

    def add(self, gt, labels):
        """conf += the counts of one image: uint8 [H, W] ground truth (numpy or torch) against uint8 [H, W] labels."""
        labels = torch.as_tensor(labels)
        device = pick_device(self.device, labels)
        g = torch.as_tensor(gt).to(device)
        assert tuple(g.shape) == tuple(labels.shape), f"Dismatch shape {tuple(g.shape)} and {tuple(labels.shape)}"
        if self._conf is None:
            self._conf, self._stray = imagelabels_ops.new_confusion(self.num_classes, device)
        imagelabels_ops.label_confusion(g.to(torch.uint8), labels.to(device=device, dtype=torch.uint8), self.num_classes, self.ignore_label,
                                        self._conf, self._stray)
        self._processed += 1

    def _read(self, path, device):
        g = device_stack([path], self.reader, device)
        return g[0] if g is not None else read_png(path)

    def process(self, inputs, outputs):
        from ..inference.results import semseg_labels_of
        for item, output in zip(inputs, outputs):
            labels = semseg_labels_of(output)
            self.add(self._read(self.gt_path(item), pick_device(self.device, labels)), labels)

    def evaluate(self):
        if self._conf is None:
            return {}
        imagelabels_ops.raise_on_stray(self._stray, self.num_classes, self.ignore_label)
        res = semseg_scores(self._conf.cpu().numpy(), self.class_names)
        if self._output_dir:
            save_dir = os.path.join(self._output_dir, "inference")
            os.makedirs(save_dir, exist_ok=True)
            with open(os.path.join(save_dir, "sem_seg_evaluation.json"), "w") as f:
                json.dump(res, f)
        return OrderedDict(sem_seg=res)


def evaluate_semseg_files(sem_dir, sem_gt_dir, num_classes, ignore_label=255, class_names=None, device=None, reader="host"):
    """mIoU of class-id PNGs already on disk: every PNG of `sem_dir` against the file of its name in `sem_gt_dir`.  The predictions hold
    the same kind of value as the ground truth (contiguous classes)."""
    ev = SemSegEvaluator(sem_gt_dir, num_classes, ignore_label, class_names, device=device, reader=reader)
    device = pick_device(device)
    for name in sorted(n for n in os.listdir(sem_dir) if n.endswith(".png")):
        ev.add(ev._read(os.path.join(sem_gt_dir, name), device), torch.as_tensor(ev._read(os.path.join(sem_dir, name), device)))
    return ev.evaluate()


def main(argv=None):
    ap = argparse.ArgumentParser(description="PQ of panoptic PNGs, or mIoU of class-id PNGs, already on disk")
    ap.add_argument("--panoptic_dir", help="the predicted panoptic PNGs (predictions.json beside the folder, or --predictions_json)")
    ap.add_argument("--predictions_json")
    ap.add_argument("--pan_gt_json", help="the ground truth in COCO's panoptic format")
    ap.add_argument("--truth_dir", help="the folder of the ground-truth panoptic PNGs")
    ap.add_argument("--sem_dir", help="the predicted class-id PNGs")
    ap.add_argument("--sem_gt_dir", help="the ground-truth class-id PNGs, named alike")
    ap.add_argument("--num_classes", type=int)
    ap.add_argument("--ignore_label", type=int, default=255)
    ap.add_argument("--device", default=None, help="cuda / cpu (default: the GPU when there is one)")
    ap.add_argument("--reader", default="host", choices=("host", "gpu"), help="who decodes the PNGs: Pillow on the host, or the device")
    a = ap.parse_args(argv)
    if (a.panoptic_dir is None) == (a.sem_dir is None):
        ap.error("give either --panoptic_dir (with --pan_gt_json and --truth_dir) or --sem_dir (with --sem_gt_dir and --num_classes)")
    if a.panoptic_dir is not None:
        if not (a.pan_gt_json and a.truth_dir):
            ap.error("--panoptic_dir needs --pan_gt_json and --truth_dir")
        r = evaluate_panoptic_files(a.panoptic_dir, a.pan_gt_json, a.truth_dir, a.predictions_json, a.device, a.reader)
        print(pq_final_text(r["panoptic_seg"]), end="")
    else:
        if not (a.sem_gt_dir and a.num_classes):
            ap.error("--sem_dir needs --sem_gt_dir and --num_classes")
        r = evaluate_semseg_files(a.sem_dir, a.sem_gt_dir, a.num_classes, a.ignore_label, device=a.device, reader=a.reader)
        print("".join("%s:%.4f\n" % (k, r["sem_seg"][k]) for k in ("mIoU", "fwIoU", "mACC", "pACC")), end="")
    return r


if __name__ == "__main__":
    main()
