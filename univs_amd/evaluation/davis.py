"""J (region similarity), F (boundary measure) and their mean / recall / decay of a DAVIS-format VOS result, from one count per video
(davis_counts.py) instead of two OpenCV dilations per (gt object, result object, frame).

The reference scores the PNGs that its VOS / referring-VOS drivers write with `DAVISEvaluator` / `evaluate_davis`
(univs/evaluation/vos_davis_evaluation.py:35-239) over the vendored davis2017 package (univs/evaluation/davis2017_evaluation/davis2017:
davis.py, results.py, metrics.py, utils.py).  Both scores are ratios of exact integer counts, which `davis_counts` takes from the two
uint8 stacks of a sequence in one launch for every pair of objects; the rest is host arithmetic in float64 with the reference's own
expressions on the same integers, so the numbers and the result text come out the same.

  disk_radius            the dilation radius of a frame size (metrics.py:77-78)
  jf_from_counts         per-frame J and F of every pair from the integer counts, with the reference's special cases
  db_statistics          mean, recall (share above 0.5) and decay of a per-frame series (utils.py:136-162)
  read_sequence          the annotation maps of one sequence, with the DAVIS directory rules
  evaluate_davis_files   the file-level entry point: every PNG read once, one upload and one `davis_counts` call per sequence
  DAVISEvaluator         reset / process / evaluate with the reference's call pattern

Reproduced on purpose: the semi-supervised task drops the first and the last frame and ignores the void label; the number of gt objects
is the maximum of the FIRST frame, the number of result objects the maximum over all frames read; the unsupervised task names the
matched rows `<seq>_<k>` in the order of the matched proposals; with one metric only it fails on an undefined name (NameError);
`db_statistics` casts its bin edges to uint8, so they wrap for sequences longer than 256 frames; `davis-metrics.txt` has no line ends.

`python -m univs_amd.evaluation.davis --res_path ... --davis_root ... --task ...` scores a result directory.  Single process.
"""
import argparse
import glob
import os
import sys
import warnings

import numpy as np
import torch

from ._counts import check_reader, device_stack, pick_device as _device, read_png as _read
from .davis_counts import davis_counts

SUBSET_OPTIONS = ("train", "val", "test-dev", "test-challenge")
TASKS = ("semi-supervised", "unsupervised")
VOID_LABEL = 255
MAX_PROPOSALS = 20


def disk_radius(H, W, bound_th=0.008):
    """The radius `f_measure` dilates with: `bound_th` itself when it is >= 1, else ceil(bound_th * |(H, W)|): 8 at 480 x 854."""
    return int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((H, W))))


def jf_from_counts(region, n_gt, n_fg, match):
    """(J, F), float64 [G, P, T], from the integer counts of `davis_counts` (tensors or arrays).

    J = intersection / max(union, 1), 1 where the union is empty (metrics.py:32-36).  F = 2 p r / (p + r) with precision p = matched
    result boundary pixels / result boundary pixels and recall r its mirror image; an empty result boundary gives (1, 0), an empty gt
    boundary (0, 1), both empty (1, 1); F = 0 where p + r = 0 (metrics.py:100-117)."""
    region, n_gt, n_fg, match = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x).astype(np.int64) for x in (region, n_gt, n_fg, match))
    inters, union = region[..., 0], region[..., 1]
    J = inters / np.clip(union, 1, None)
    J[union == 0] = 1
    ng = np.broadcast_to(n_gt[:, None, :], inters.shape)
    nf = np.broadcast_to(n_fg[None, :, :], inters.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = match[..., 1] / nf.astype(np.float64)
        recall = match[..., 0] / ng.astype(np.float64)
    precision = np.where(nf == 0, 1.0, np.where(ng == 0, 0.0, precision))
    recall = np.where(nf == 0, np.where(ng == 0, 1.0, 0.0), np.where(ng == 0, 1.0, recall))
    with np.errstate(divide="ignore", invalid="ignore"):
        F = np.where(precision + recall == 0, 0.0, 2 * precision * recall / (precision + recall))
    return J, F


def db_statistics(per_frame_values):
    """(mean, recall, decay) of a per-frame series: nan-mean, nan-mean of `> 0.5`, and the nan-mean of the first of four bins minus that
    of the last.  The bin edges round(linspace(1, n, 5) + 1e-10) - 1 go through uint8, as the reference has them: beyond 256 frames they
    wrap."""
    v = np.asarray(per_frame_values)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        M = np.nanmean(v)
        O = np.nanmean(v > 0.5)
        ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.uint8)
        bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
        D = np.nanmean(bins[0]) - np.nanmean(bins[3])
    return M, O, D


# ------------------------------------------------------------------------------------------------------------------------------------
# the DAVIS tree
# ------------------------------------------------------------------------------------------------------------------------------------
def _paths(davis_root, task, subset, resolution):
    if subset not in SUBSET_OPTIONS:
        raise ValueError(f"Subset should be in {list(SUBSET_OPTIONS)}")
    if task not in TASKS:
        raise ValueError(f"The only tasks that are supported are {list(TASKS)}")
    img_path = os.path.join(davis_root, "JPEGImages", resolution)
    mask_path = os.path.join(davis_root, "Annotations" if task == "semi-supervised" else "Annotations_unsupervised", resolution)
    year = "2019" if task == "unsupervised" and subset in ("test-dev", "test-challenge") else "2017"
    return img_path, mask_path, os.path.join(davis_root, "ImageSets", year, f"{subset}.txt")


def list_sequences(davis_root, task, subset="val", sequences="all", resolution="480p"):
    """The sequence names of a DAVIS tree, as `DAVIS.__init__` collects them (davis.py:14-63): the lines of ImageSets/<year>/<subset>.txt
    for 'all', else the given name(s).  FileNotFoundError for a missing root, subset list, annotation folder (train / val) or a
    sequence without JPEG images."""
    img_path, mask_path, set_file = _paths(davis_root, task, subset, resolution)
    if not os.path.exists(davis_root):
        raise FileNotFoundError(f"DAVIS not found in {davis_root}")
    if not os.path.exists(set_file):
        raise FileNotFoundError(f"Subset sequences list for {subset} not found: {set_file}")
    if subset in ("train", "val") and not os.path.exists(mask_path):
        raise FileNotFoundError(f"Annotations folder for the {task} task not found: {mask_path}")
    if sequences == "all":
        with open(set_file, "r") as f:
            names = [x.strip() for x in f.readlines()]
    else:
        names = list(sequences) if isinstance(sequences, (list, tuple)) else [sequences]
    for seq in names:
        if not glob.glob(os.path.join(img_path, seq, "*.jpg")):
            raise FileNotFoundError(f"Images for sequence {os.path.join(img_path, seq)} not found.")
    return names


def read_sequence(davis_root, seq, task, resolution="480p", reader="host", device=None):
    """(maps uint8 [T, H, W], frame ids) of one sequence: the sorted `*.png` files of Annotations[_unsupervised]/<resolution>/<seq>, raw
    (255 = void is still in them).  JPEGImages/<resolution>/<seq>/*.jpg must exist and fixes the frame count: fewer annotations than
    images is a FileNotFoundError here (the reference fails on the missing file's placeholder).  A frame id is the file name without
    its extension and without dots.  Frames of another size than the first are a ValueError, as the reference's array assignment.
    reader "gpu": the maps are decoded on the device and returned as a device tensor (`_counts.device_stack`; files it does not take go
    through the loop below)."""
    img_path, mask_path, _ = _paths(davis_root, task, "val", resolution)
    images = sorted(glob.glob(os.path.join(img_path, seq, "*.jpg")))
    if not images:
        raise FileNotFoundError(f"Images for sequence {os.path.join(img_path, seq)} not found.")
    masks = sorted(glob.glob(os.path.join(mask_path, seq, "*.png")))
    if len(masks) < len(images):
        raise FileNotFoundError(f"{len(masks)} annotations for the {len(images)} images of {os.path.join(mask_path, seq)}")
    stack = device_stack(masks, reader, device)
    if stack is not None:
        return stack, ["".join(m.split("/")[-1].split(".")[:-1]) for m in masks]
    maps, ids = [], []
    for m in masks:
        a = _read(m)
        if a.ndim != 2 or a.dtype != np.uint8 or (maps and a.shape != maps[0].shape):
            raise ValueError(f"{m}: {a.dtype} {a.shape} is no uint8 id map of the sequence's size")
        maps.append(a)
        ids.append("".join(m.split("/")[-1].split(".")[:-1]))
    return np.stack(maps), ids


def read_results(res_path, seq, frame_ids, reader="host", device=None):
    """uint8 [T, H, W]: `<res_path>/<seq>/<frame id>.png` of every id (results.py:11-26).  A file that cannot be read ends the run
    (SystemExit), a frame of another size than the first is a ValueError.  reader "gpu": as in `read_sequence`."""
    stack = device_stack([os.path.join(res_path, seq, f"{fid}.png") for fid in frame_ids], reader, device)
    if stack is not None:
        return stack
    maps = []
    for fid in frame_ids:
        path = os.path.join(res_path, seq, f"{fid}.png")
        try:
            a = _read(path)
        except IOError as err:
            sys.stdout.write(f"{seq} frame {fid} not found! {path} \n")
            sys.stderr.write(f"IOError: {err.strerror}\n")
            sys.exit()
        if a.ndim != 2 or a.dtype != np.uint8 or (maps and a.shape != maps[0].shape):
            raise ValueError(f"{path}: {a.dtype} {a.shape} is no uint8 id map of the sequence's size")
        maps.append(a)
    return np.stack(maps)


# ------------------------------------------------------------------------------------------------------------------------------------
# scoring
# ------------------------------------------------------------------------------------------------------------------------------------
def sequence_tables(gt, pred, task, metrics=("J", "F"), device=None, bound_th=0.008):
    """(j, f), float64 [G, T'] each: the per-frame series of the gt objects of one sequence, as `_evaluate_semisupervised` /
    `_evaluate_unsupervised` return them (vos_davis_evaluation.py:198-239).  gt uint8 [T, H, W] raw (with its 255s, all frames), pred
    uint8 [T', H', W'] the result frames that the task reads (T' = T - 2 in the semi-supervised task).  One upload of the two stacks,
    one `davis_counts` call, one transfer of the counts back."""
    if isinstance(gt, torch.Tensor) != isinstance(pred, torch.Tensor):              # (reader "gpu" and one side went through the host loop)
        gt, pred = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (gt, pred))
    on_device = isinstance(gt, torch.Tensor)                         # (reader "gpu": both stacks are there already)
    G = int((gt[0] * (gt[0] != VOID_LABEL)).max()) if on_device else int(np.where(gt[0] == VOID_LABEL, 0, gt[0]).max())   # the first frame of the whole sequence decides
    if task == "semi-supervised":
        gt = gt[1:-1]
    P = int(pred.max())
    if task == "unsupervised" and P > MAX_PROPOSALS:
        sys.stdout.write(f"\nIn your PNG files there is an index higher than the maximum number ({MAX_PROPOSALS}) of proposals allowed!")
        sys.exit()
    if task == "semi-supervised" and P > G:
        sys.stdout.write("\nIn your PNG files there is an index higher than the number of objects in the sequence!")
        sys.exit()
    T = gt.shape[0]
    if G == 0:
        return np.zeros((0, T)), np.zeros((0, T))
    if "J" in metrics or "F" in metrics:
        assert gt.shape == pred.shape, f"Annotation({tuple(gt.shape)}) and segmentation:{tuple(pred.shape)} dimensions do not match."
    Pp = max(P, G)                                                   # missing result objects are empty masks
    device = _device(device)
    if on_device:
        g_dev, p_dev = gt.contiguous().to(device), pred.contiguous().to(device)
    else:
        g_dev, p_dev = torch.as_tensor(np.ascontiguousarray(gt)).to(device), torch.as_tensor(np.ascontiguousarray(pred)).to(device)
    counts = davis_counts(g_dev, p_dev, G, Pp, disk_radius(gt.shape[1], gt.shape[2], bound_th), task == "unsupervised")
    flat = torch.cat([c.reshape(-1) for c in counts]).cpu().numpy()
    sizes = [int(c.numel()) for c in counts]
    parts = np.split(flat, np.cumsum(sizes)[:-1])
    J, F = jf_from_counts(*(p.reshape(tuple(c.shape)) for p, c in zip(parts, counts)))
    # a metric that was not asked for stays zero, as the reference's tables
    j = np.ascontiguousarray(J.transpose(1, 0, 2)) if "J" in metrics else np.zeros((Pp, G, T))     # [result, gt, frame]
    f = np.ascontiguousarray(F.transpose(1, 0, 2)) if "F" in metrics else np.zeros((Pp, G, T))
    if task == "semi-supervised":
        k = np.arange(G)
        return j[k, k], f[k, k]
    if not ("J" in metrics and "F" in metrics):
        raise NameError("name 'metric' is not defined")             # the reference's single-metric branch (:236)
    from scipy.optimize import linear_sum_assignment
    both = (np.mean(j, axis=2) + np.mean(f, axis=2)) / 2
    rows, cols = linear_sum_assignment(-both)
    return j[rows, cols, :], f[rows, cols, :]


def metrics_text(metrics_res):
    """The text of davis-metrics.txt (vos_davis_evaluation.py:142-150): no line ends."""
    out = []
    for m, m_res in metrics_res.items():
        out.append(f"Saving metric {m}")
        for k, v in m_res.items():
            if k in {"M", "R", "D"}:
                v = sum(v) / len(v) * 100.
                out.append(f"{k} : {v}")
    return "".join(out)


def evaluate_davis_files(davis_root, res_path, task, subset="val", sequences="all", resolution="480p", metrics=("J", "F"), device=None,
                         output_dir=None, reader="host"):
    """`evaluate_davis` on a DAVIS tree and a result directory `<res_path>/<seq>/<frame id>.png`: {"J": {"M", "R", "D": one entry per
    scored object, "M_per_object": {"<seq>_<k>": mean}}, "F": the same}.  Every PNG is read once; a sequence's two stacks are uploaded
    once to `device` (default: the GPU when there is one, else the ATen counts on the CPU).  Writes davis-metrics.txt into `output_dir`
    when it is given.  reader "gpu": the PNGs are decoded on the device (`_counts.device_stack`) instead of by Pillow.

    Errors as the reference's: SystemExit for a result frame that cannot be read, a result id above the number of gt objects
    (semi-supervised) or above 20 (unsupervised); AssertionError for result frames of another size than the annotations;
    FileNotFoundError for a missing tree; NameError for the unsupervised task with one metric only."""
    metrics = tuple(metrics) if isinstance(metrics, (tuple, list)) else (metrics,)
    check_reader(reader)
    if "T" in metrics:
        raise ValueError("Temporal metric not supported!")
    if "J" not in metrics and "F" not in metrics:
        raise ValueError("Metric possible values are J for IoU or F for Boundary")
    metrics_res = {}
    for m in ("J", "F"):
        if m in metrics:
            metrics_res[m] = {"M": [], "R": [], "D": [], "M_per_object": {}}
    for seq in list_sequences(davis_root, task, subset, sequences, resolution):
        gt, ids = read_sequence(davis_root, seq, task, resolution, reader, device)
        if task == "semi-supervised":
            ids = ids[1:-1]
        ids[0]                                                       # (no frame left: the reference's IndexError)
        pred = read_results(res_path, seq, ids, reader, device)
        j, f = sequence_tables(gt, pred, task, metrics, device)
        for ii in range(j.shape[0]):
            for m, table in (("J", j), ("F", f)):
                if m in metrics:
                    M, R, D = db_statistics(table[ii])
                    metrics_res[m]["M"].append(M)
                    metrics_res[m]["R"].append(R)
                    metrics_res[m]["D"].append(D)
                    metrics_res[m]["M_per_object"][f"{seq}_{ii + 1}"] = M
    if output_dir is not None:
        if output_dir:
            os.makedirs(output_dir, exist_ok=True)
        with open(os.path.join(output_dir, "davis-metrics.txt"), "w") as fh:
            fh.write(metrics_text(metrics_res))
    return metrics_res


class DAVISEvaluator:
    """The reference's `DAVISEvaluator` (vos_davis_evaluation.py:35-150) with the dataset's `image_root` as an explicit argument in place
    of detectron2's MetadataCatalog.  Task and resolution follow from the dataset name as there (:89-110): 'refdavis' is the
    unsupervised task at 480p with the ground truth in `<image_root minus two components>/DAVIS`, 'davis16' / 'davis17' the
    semi-supervised task at Full-Resolution in `<image_root minus two components>`.  `process` is empty, as in the reference: the
    driver has already written the PNGs to `<output_dir>/Annotations`."""

    def __init__(self, dataset_name, image_root, tasks=None, output_dir=None, gt_set="val", sequences="all", metrics=("J", "F"), device=None,
                 reader="host"):
        self.reader = check_reader(reader)                           # ("host" | "gpu": who decodes the PNGs, _counts.device_stack)
        if "refdavis" in dataset_name:
            inferred, self.resolution = "unsupervised", "480p"
            self.gt_root = "/".join(image_root.split("/")[:-2] + ["DAVIS"])
        elif "davis16" in dataset_name or "davis17" in dataset_name:
            inferred, self.resolution = "semi-supervised", "Full-Resolution"
            self.gt_root = "/".join(image_root.split("/")[:-2])
        else:
            raise ValueError(f"{dataset_name}: no DAVIS dataset name (refdavis, davis16, davis17)")
        tasks = inferred if tasks is None else tasks
        assert isinstance(tasks, (str, list)), f"invalid type: {tasks}"
        self.task = tasks if isinstance(tasks, str) else tasks[0]
        self.gt_root = os.path.join(os.getcwd(), self.gt_root)
        self.subset, self.sequences, self.device, self._output_dir = gt_set, sequences, device, output_dir
        self.metrics = metrics if isinstance(metrics, (tuple, list)) else [metrics]
        if "T" in self.metrics:
            raise ValueError("Temporal metric not supported!")
        if "J" not in self.metrics and "F" not in self.metrics:
            raise ValueError("Metric possible values are J for IoU or F for Boundary")
        list_sequences(self.gt_root, self.task, gt_set, sequences, self.resolution)     # the reference builds its DAVIS object here

    def reset(self):
        self._predictions = []
        os.makedirs(self._output_dir, exist_ok=True)

    def process(self, inputs, outputs):
        """Nothing: the VOS driver writes the PNGs itself."""

    def evaluate(self):
        """`evaluate_davis` on `<output_dir>/Annotations`; davis-metrics.txt into `output_dir`.  Returns the metrics dictionary (the
        reference returns nothing)."""
        res = evaluate_davis_files(self.gt_root, os.path.join(self._output_dir, "Annotations"), self.task, self.subset, self.sequences,
                                   self.resolution, self.metrics, self.device, self._output_dir, reader=self.reader)
        for m_res in res.values():
            for k in ("M", "R", "D"):
                print("{}: {:.2f}".format(k, sum(m_res[k]) / len(m_res[k]) * 100.))
        return res


def main(argv=None):
    ap = argparse.ArgumentParser(description="J and F (mean, recall, decay) of a DAVIS-format result directory")
    ap.add_argument("--res_path", required=True, help="the result directory: <seq>/<frame id>.png")
    ap.add_argument("--davis_root", required=True, help="the DAVIS root: JPEGImages, Annotations[_unsupervised], ImageSets")
    ap.add_argument("--task", required=True, choices=TASKS)
    ap.add_argument("--subset", default="val")
    ap.add_argument("--resolution", default="480p", help="480p or Full-Resolution")
    ap.add_argument("--output_dir", default=None, help="where davis-metrics.txt goes (default: it is not written)")
    ap.add_argument("--device", default=None, help="cuda / cpu (default: the GPU when there is one)")
    ap.add_argument("--reader", default="host", choices=("host", "gpu"), help="who decodes the PNGs: Pillow on the host, or the device")
    a = ap.parse_args(argv)
    r = evaluate_davis_files(a.davis_root, a.res_path, a.task, a.subset, "all", a.resolution, ("J", "F"), a.device, a.output_dir, reader=a.reader)
    for m, m_res in r.items():
        print(m, *("{}: {:.2f}".format(k, sum(m_res[k]) / len(m_res[k]) * 100.) for k in ("M", "R", "D")))
    return r


if __name__ == "__main__":
    main()
