"""mIoU and VC8 / VC16 of a VSPW-format result, from one count per video (vss_counts.py) instead of repeated passes over the pixels.

The reference scores a result with `VSSEvaluator.evaluate` (univs/evaluation/vss_evaluation.py:120-224; the same logic as the scripts
eval_miou_vss.py and eval_vc_perclip_vss.py over eval_utils_vss.Evaluator): one pass for the confusion matrix, then for each clip length
n in (8, 16) and every window start i a comparison of frame i with each of the next n - 1 frames on both sides, over float planes.  All
three scores are ratios of exact integer counts, which `vss_counts` takes from the two uint8 stacks of a video in one launch; the rest is
host arithmetic in float64 with the reference's own expressions, so the result texts come out the same.

  score_counts         the four mIoU figures of the summed confusion matrix, and per n `np.nanmean` of the per-window ratios
  evaluate_vss_files   the file-level entry point: every PNG read once, one upload and one `vss_counts` call per video
  VSSEvaluator         reset / process / evaluate with the reference's call pattern; `process` counts the video from the tensors it
                       is handed, so `evaluate` does not re-read the PNGs it wrote

Reproduced on purpose: windows are `range(T - n)`, so the last window that fits is not scored; a video is skipped when its mask directory
has <= n entries (dot files counted); video and file names that start with "." are left out of the VC pass only; no window at all gives
nan.  One deviation: see `read_split`.

`python -m univs_amd.evaluation.vss --submit_dir ... --data_dir ... --split_file ...` is the reference's two scripts in one.
Single process, as the reference (it scores on rank 0).
"""
import argparse
import os
import warnings

import numpy as np
import torch

from ._counts import check_reader, device_stack, pick_device as _device, read_png as _read, stack as _stack
from .vss_counts import CLIP_NUMS, vss_counts


class VideoCounts:
    """One video of the split: `name`, its mask directory's number of `entries` (dot files included, what the reference's length test
    sees), `confusion` int64 [C, C] over every mask file, and `windows` int64 [T, 2, 2] over the files whose names do not start with "."
    in sorted order (None for a video the VC pass never looks at)."""

    def __init__(self, name, entries, confusion, windows):
        self.name, self.entries = name, int(entries)
        self.confusion = np.asarray(confusion, dtype=np.int64)
        self.windows = None if windows is None else np.asarray(windows, dtype=np.int64)


def miou_scores(confusion):
    """(Acc, Acc_class, mIoU, FWIoU) of a confusion matrix with the expressions of eval_utils_vss.Evaluator (:68-94) in float64."""
    cm = np.asarray(confusion).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        acc = np.diag(cm).sum() / cm.sum()
        acc_class = np.nanmean(np.diag(cm) / cm.sum(axis=1))
        iu = np.diag(cm) / (np.sum(cm, axis=1) + np.sum(cm, axis=0) - np.diag(cm))
        isval = np.sum(cm, axis=1) > 0
        miou = np.nansum(iu * isval) / isval.sum()
        freq = np.sum(cm, axis=1) / np.sum(cm)
        fwiou = (freq[freq > 0] * iu[freq > 0]).sum()
    return acc, acc_class, miou, fwiou


def window_ratios(videos, clip_num):
    """The list that `evaluate_vc_perclip` collects for one clip length (vss_evaluation.py:187-212): one num / den per scored window
    (0 / 0 -> nan), videos in split order, windows in order."""
    k = CLIP_NUMS.index(clip_num)
    out = []
    for v in videos:
        if v.name[0] == "." or v.entries <= clip_num:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(len(v.windows) - clip_num):               # the reference's range: the last window that fits is left out
                out.append(v.windows[i, k, 1] / v.windows[i, k, 0])
    return out


def score_counts(per_video_counts, split_name, output_dir=None, num_classes=124):
    """The scores of a split from its videos' counts (VideoCounts, in split order), and the reference's three result files into
    `output_dir` when it is given: {"Acc", "Acc_class", "mIoU", "FWIoU", "VC8", "VC16", "confusion" int64 [C, C], "ratios": {n: float64
    array}, "files": {file name: text}}.  `num_classes` matters for an empty split only: the reference's untouched zero matrix."""
    videos = list(per_video_counts)
    confusion = np.zeros((num_classes, num_classes), dtype=np.int64)
    if videos:
        confusion = np.sum([v.confusion for v in videos], axis=0, dtype=np.int64)
    acc, acc_class, miou, fwiou = miou_scores(confusion)
    out = {"Acc": acc, "Acc_class": acc_class, "mIoU": miou, "FWIoU": fwiou, "confusion": confusion, "ratios": {}, "files": {}}
    out["files"]["miou-final.txt"] = "Acc:{}, Acc_class:{}, mIoU:{}, fwIoU: {}".format(acc, acc_class, miou, fwiou)
    for n in CLIP_NUMS:
        ratios = np.array(window_ratios(videos, n))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # (mean of an empty list: nan, as the reference prints it)
            vc = np.nanmean(ratios)                                  # on the one list: a running sum differs in the last digit
        out["VC%d" % n], out["ratios"][n] = vc, ratios
        out["files"]["vc%d-final.txt" % n] = "VC{} score: {} on {} set".format(n, vc, split_name)
    if output_dir is not None:
        if output_dir:
            os.makedirs(output_dir, exist_ok=True)
        for name, text in out["files"].items():
            with open(os.path.join(output_dir, name), "w") as f:
                f.write(text)
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# counts of a video, and the file-level entry points
# ------------------------------------------------------------------------------------------------------------------------------------
def _count(gt, pred, num_classes, device):
    """numpy / torch uint8 [T, H, W] stacks -> (confusion, windows) as int64 numpy; the reference's ValueError on the overflow flag."""
    g = torch.as_tensor(gt).to(device)
    p = torch.as_tensor(pred).to(device)
    confusion, windows, overflow = vss_counts(g, p, num_classes)
    over = int(overflow.item())
    if over >= 0:
        raise ValueError(f"cannot reshape array of size {over + 1} into shape ({num_classes},{num_classes})")
    return confusion.cpu().numpy().astype(np.int64), windows.cpu().numpy().astype(np.int64)


def read_split(data_dir, split_file):
    """The video names of `data_dir/split_file`, one per line.  A line loses its line ending only: the reference's `line[:-1]` also eats
    the last character of a final line that has no line ending (the one deviation of this module)."""
    with open(os.path.join(data_dir, split_file), "r") as f:
        return [line.rstrip("\n") for line in f.readlines()]


def video_counts(name, entries, frames, num_classes, device=None):
    """VideoCounts from `frames` = [(file name, gt uint8 [H, W], pred uint8 [H, W])] in any order: the files whose names start with "."
    count for the confusion matrix only; the others are stacked in sorted order and counted in one `vss_counts` call."""
    device = _device(device)
    confusion = np.zeros((num_classes, num_classes), dtype=np.int64)
    windows = None
    plain = sorted((f for f in frames if f[0][0] != "."), key=lambda f: f[0])
    if plain:
        c, windows = _count(_stack([f[1] for f in plain]), _stack([f[2] for f in plain]), num_classes, device)
        confusion += c
    for f in frames:
        if f[0][0] == ".":
            confusion += _count(f[1][None], f[2][None], num_classes, device)[0]
    if name[:1] == ".":
        windows = None
    elif windows is None:
        windows = np.zeros((0, 2, 2), dtype=np.int64)
    return VideoCounts(name, entries, confusion, windows)


def _counts_from_files(video, submit_dir, data_dir, num_classes, device, reader="host"):
    """One video read as `evaluate_miou` reads it (vss_evaluation.py:140-159): the mask directory's entries in listing order, the ground
    truth before the prediction, the size assertion per file.  When a file fails, the files before it are counted first: the reference
    would have met their ValueError earlier.  reader "gpu": the two sides are decoded on the device, one call each; a video with a
    file that is missing, of another size or not decoded there goes through the loop below."""
    mask_dir = os.path.join(data_dir, "data", video, "mask")
    listing = os.listdir(mask_dir)
    g = device_stack([os.path.join(mask_dir, tar) for tar in listing], reader, device)
    p = device_stack([os.path.join(submit_dir, video, tar) for tar in listing], reader, device) if g is not None else None
    if p is not None and g.shape == p.shape:
        return video_counts(video, len(listing), [(tar, g[i], p[i]) for i, tar in enumerate(listing)], num_classes, device)
    frames, failure = [], None
    for tar in listing:
        try:
            g = _read(os.path.join(mask_dir, tar))
            p = _read(os.path.join(submit_dir, video, tar))
            assert g.shape[-2:] == p.shape[-2:], "Mismatch shapes between predicted and GT masks"
        except (OSError, AssertionError) as e:
            failure = e
            break
        frames.append((tar, g, p))
    if failure is not None:
        for f in frames:
            _count(f[1][None], f[2][None], num_classes, device)
        raise failure
    return video_counts(video, len(listing), frames, num_classes, device)


def evaluate_vss_files(submit_dir, data_dir, split_file="val.txt", num_classes=124, device=None, output_dir=None, reader="host"):
    """`VSSEvaluator.evaluate` (and the two scripts) on a VSPW tree: the videos of `data_dir/split_file`, the ground truth in
    `data_dir/data/<video>/mask/*.png`, the predictions in `submit_dir/<video>/<name>.png`.  Every PNG is read once into one uint8 stack
    per side and video, counted by one `vss_counts` call on `device` (default: the GPU when there is one).  Writes miou-final.txt,
    vc8-final.txt and vc16-final.txt into `output_dir` (default: `submit_dir`, as the scripts) and returns `score_counts`' dict.
    reader "gpu": the PNGs are decoded on the device (`_counts.device_stack`) instead of by Pillow.

    Errors as the reference's, mIoU first: a prediction of another size is an AssertionError, a missing one a FileNotFoundError, a
    confusion cell beyond num_classes^2 a ValueError.  Split lines: see `read_split`."""
    device = _device(device)
    check_reader(reader)
    videos = [_counts_from_files(v, submit_dir, data_dir, num_classes, device, reader) for v in read_split(data_dir, split_file)]
    return score_counts(videos, split_file, submit_dir if output_dir is None else output_dir, num_classes)


class VSSEvaluator:
    """The reference's `VSSEvaluator` (vss_evaluation.py) with explicit arguments in place of detectron2's MetadataCatalog:
    `contiguous_id_to_dataset_id` and `ignore_val` (for the PNGs), `num_classes`, the VSPW root `data_dir` with its `split_file`, and
    `output_dir`, where the PNGs go; the three result files go to its parent, as the reference's evaluator has it.

    `process` writes the video's PNGs through `results.write_vss_predictions`, unchanged.  When the names it wrote are exactly the names
    in the video's mask directory, it also counts the video at once from the tensor it was handed and the ground-truth masks; `evaluate`
    then reads no PNG of that video.  Any other video of the split is scored from the files."""

    def __init__(self, contiguous_id_to_dataset_id, ignore_val, num_classes, data_dir, split_file, output_dir, device=None, eval_miou_res=-1, png="host",
                 reader="host"):
        if eval_miou_res > 0:
            raise NotImplementedError("eval_miou_res > 0 rescales the ground truth with mmcv, which the reference's evaluator does not import")
        self.contiguous_id_to_dataset_id, self.ignore_val, self.num_classes = dict(contiguous_id_to_dataset_id), ignore_val, int(num_classes)
        self.data_dir, self.split_file, self._output_dir, self.device = data_dir, split_file, output_dir, device
        self.png = png                                               # ("host" | "gpu": who compresses the PNGs, results.py)
        self.reader = check_reader(reader)                           # ("host" | "gpu": who decodes them, _counts.device_stack)
        self.reset()

    def reset(self):
        self._processed, self._counts = 0, {}
        os.makedirs(self._output_dir, exist_ok=True)

    def process(self, inputs, outputs):
        from ..inference.results import write_vss_predictions
        assert len(inputs) == 1, "More than one inputs are loaded for inference!"
        paths = write_vss_predictions(inputs[0], outputs, self._output_dir, self.contiguous_id_to_dataset_id, self.ignore_val, png=self.png)
        self._processed += 1
        video = str(inputs[0]["video_id"])
        self._counts.pop(video, None)
        counts = self._counts_in_process(video, [os.path.basename(p) for p in paths], outputs)
        if counts is not None:
            self._counts[video] = counts

    def _png_bytes(self, sem, device):
        """What `write_vss_predictions` paints, on the device: the dataset id minus the smallest one, 255 for the ignore value."""
        lut = torch.full((256,), 255, dtype=torch.uint8)
        lo = min(self.contiguous_id_to_dataset_id.values())
        for c, d in self.contiguous_id_to_dataset_id.items():
            if 0 <= int(c) < 256 and int(c) != self.ignore_val:
                lut[int(c)] = (int(d) - lo) % 256
        return lut.to(device)[sem.to(device).to(torch.uint8).long()]

    def _counts_in_process(self, video, names, outputs):
        mask_dir = os.path.join(self.data_dir, "data", video, "mask")
        if not os.path.isdir(mask_dir):
            return None
        listing = os.listdir(mask_dir)
        if sorted(listing) != sorted(names) or len(set(names)) != len(names) or any(n[0] == "." for n in names):
            return None                                              # evaluate() would read other files than the ones just written
        sem = outputs["pred_masks"]
        sem = sem if isinstance(sem, torch.Tensor) else torch.as_tensor(np.asarray(sem))
        order = sorted(range(len(names)), key=lambda i: names[i])
        device = _device(self.device, sem)
        gt = device_stack([os.path.join(mask_dir, names[i]) for i in order], self.reader, device)
        if gt is None:
            gt = [_read(os.path.join(mask_dir, names[i])) for i in order]
            if any(g.ndim != 2 or g.dtype != np.uint8 or tuple(g.shape) != tuple(sem.shape[1:]) for g in gt):
                return None                                          # (evaluate() raises the reference's size assertion from the files)
            gt = np.stack(gt)
        elif tuple(gt.shape[1:]) != tuple(sem.shape[1:]):
            return None
        pred = self._png_bytes(sem, device)[torch.as_tensor(order, device=device)]
        try:
            confusion, windows = _count(gt, pred, self.num_classes, device)
        except ValueError:
            return None                                              # (raised by evaluate(), from the files, in the split's order)
        return VideoCounts(video, len(listing), confusion, windows)

    def evaluate(self):
        """The reference's `evaluate_miou` + `evaluate_vc_perclip`: `score_counts`' dict, the files in the parent of `output_dir`."""
        device = _device(self.device)
        videos = []
        for v in read_split(self.data_dir, self.split_file):
            c = self._counts.get(v)
            videos.append(c if c is not None else _counts_from_files(v, self._output_dir, self.data_dir, self.num_classes, device, self.reader))
        return score_counts(videos, self.split_file, "/".join(self._output_dir.split("/")[:-1]), self.num_classes)


def main(argv=None):
    ap = argparse.ArgumentParser(description="mIoU and VC8 / VC16 of a VSPW-format result directory")
    ap.add_argument("--submit_dir", "-i", required=True, help="the result directory: <video>/<frame>.png")
    ap.add_argument("--data_dir", default="datasets/VSPW_480p/", help="the VSPW root: <split file>, data/<video>/mask/<frame>.png")
    ap.add_argument("--split_file", default="val.txt", help="val.txt or test.txt")
    ap.add_argument("--num_classes", type=int, default=124)
    ap.add_argument("--device", default=None, help="cuda / cpu (default: the GPU when there is one)")
    ap.add_argument("--reader", default="host", choices=("host", "gpu"), help="who decodes the PNGs: Pillow on the host, or the device")
    a = ap.parse_args(argv)
    r = evaluate_vss_files(a.submit_dir, a.data_dir, a.split_file, a.num_classes, a.device, reader=a.reader)
    for text in r["files"].values():
        print(text)
    return r


if __name__ == "__main__":
    main()
