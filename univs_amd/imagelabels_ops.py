"""Wrappers of the seventeenth header (include/univs_imagelabels_hip.h): a per-image semantic result as labels, and their confusion matrix.

  semseg_labels        uint8 [H, W] = argmax_c bilinear(r [C, hi, wi] -> H x W), the [C, H, W] tensor never built (csrc/semseg_labels.hip)
  label_confusion_u8   adds the pixels of two uint8 maps to an int64 [(K + 1), (K + 1)] matrix, row = ground truth (ignore -> K)
  label_confusion_aten the same matrix from an ATen `bincount`: the CPU's form, and the one beyond the kernel's (K + 1)^2 <= 32768 cells
  label_confusion      whichever of the two covers the call, and the ValueError for stray bytes

The two kernel wrappers run behind `ops._call`: GPU tensors only (a CPU tensor raises), None where the kernel does not cover the call.
inference/semseg_labels_rule.py states both in numpy and is the yardstick.
"""
import torch

from . import _lib, ops
from .inference.semseg_labels_rule import check_stray

MAX_CLASSES = 256            # semseg_labels: a class is one byte
MAX_CELLS = 32768            # label_confusion_u8: (K + 1)^2 int32 cells in 128 KB of LDS


def semseg_labels(r, out_size):
    """uint8 [H, W] of float32 r [C, hi, wi] on its device and current stream: `ops.bilinear_resample(r, out_size).argmax(0)` byte for
    byte, the first maximum winning.  None beyond C <= 256, H W < 2^31, hi wi < 2^31: the caller keeps the dense formulation."""
    name = "semseg_labels"
    ops._inference_only(name, r)
    ops._require_gpu(name, r)
    H, W = (int(v) for v in out_size)
    if r.dtype != torch.float32 or r.dim() != 3 or min(r.shape) < 1 or H < 1 or W < 1:
        raise RuntimeError(f"{name}: float32 [C, hi, wi] and a size (H, W), got {r.dtype} {tuple(r.shape)} -> {(H, W)}")
    C, hi, wi = (int(v) for v in r.shape)
    if C > MAX_CLASSES or H * W >= 2 ** 31 or hi * wi >= 2 ** 31:
        return None                                                  # (the entry's answer, without allocating what it would not write)
    labels = torch.empty((H, W), dtype=torch.uint8, device=r.device)
    ok = ops._call(name, _lib.load().univs_semseg_labels_f32, r, ops._ptr(r), C, hi, wi, H, W, ops._ptr(labels))
    return labels if ok else None


def _check_maps(name, gt, pred, num_classes, ignore_label):
    if gt.dtype != torch.uint8 or pred.dtype != torch.uint8 or gt.shape != pred.shape:
        raise RuntimeError(f"{name}: two uint8 maps of one shape, got {gt.dtype} {tuple(gt.shape)} and {pred.dtype} {tuple(pred.shape)}")
    K, ignore = int(num_classes), int(ignore_label)
    if K < 1 or not (ignore == -1 or K <= ignore <= 255):
        raise RuntimeError(f"{name}: num_classes={K} ignore_label={ignore} (-1, or a byte that is no class)")
    return K, ignore


def new_confusion(num_classes, device):
    """(conf int64 [(K + 1), (K + 1)], stray int64 [2]) of zeros: what the two counting calls add to."""
    K = int(num_classes)
    return torch.zeros((K + 1, K + 1), dtype=torch.int64, device=device), torch.zeros(2, dtype=torch.int64, device=device)


def label_confusion_u8(gt, pred, num_classes, ignore_label, conf, stray):
    """conf[row, col] += 1 for every pixel of the uint8 maps gt and pred (row = gt with ignore_label -> K, col = pred), stray += the
    pixels that fit no cell (include/univs_imagelabels_hip.h), on the maps' device and current stream.  True when it ran; None beyond
    (K + 1)^2 <= 32768 cells or n < 2^31 - 4, or for maps that do not start on a dword: nothing was added."""
    name = "label_confusion_u8"
    ops._require_gpu(name, gt, pred, conf, stray)
    K, ignore = _check_maps(name, gt, pred, num_classes, ignore_label)
    if conf.dtype != torch.int64 or tuple(conf.shape) != (K + 1, K + 1) or stray.dtype != torch.int64 or tuple(stray.shape) != (2,):
        raise RuntimeError(f"{name}: int64 conf [{K + 1}, {K + 1}] and stray [2], got {conf.dtype} {tuple(conf.shape)} and "
                           f"{stray.dtype} {tuple(stray.shape)}")
    n = gt.numel()
    if (K + 1) ** 2 > MAX_CELLS or n >= 2 ** 31 - 4:
        return None
    if n == 0:
        return True
    ok = ops._call(name, _lib.load().univs_label_confusion_u8, gt, ops._ptr(gt), ops._ptr(pred), n, K, ignore, ops._ptr(conf), ops._ptr(stray))
    return True if ok else None


def label_confusion_aten(gt, pred, num_classes, ignore_label, conf, stray):
    """The same sums from one `torch.bincount`, on any device."""
    K, ignore = _check_maps("label_confusion_aten", gt, pred, num_classes, ignore_label)
    g, p = gt.reshape(-1).long(), pred.reshape(-1).long()
    row = torch.where(g == ignore, torch.full_like(g, K), g) if ignore >= 0 else g
    bad_g = (row > K) | ((row == K) & (g != ignore))
    bad_p = ~bad_g & (p > K)
    ok = ~(bad_g | bad_p)
    conf += torch.bincount((K + 1) * row[ok] + p[ok], minlength=(K + 1) ** 2).view(K + 1, K + 1)
    stray += torch.stack([bad_g.sum(), bad_p.sum()])
    return True


def label_confusion(gt, pred, num_classes, ignore_label=255, conf=None, stray=None):
    """conf (+)= the confusion matrix of two uint8 maps, by the kernel where it covers the call and by `label_confusion_aten` elsewhere
    (the CPU; more than 32768 cells).  Given `conf` and `stray` (`new_confusion`) it accumulates and returns them without a
    read-back -- the caller checks `stray` once (`raise_on_stray`); without them it returns a fresh conf and raises the ValueError of
    a stray byte at once."""
    own = conf is None
    if own:
        conf, stray = new_confusion(num_classes, gt.device)
    gt, pred = gt.contiguous(), pred.contiguous()
    if not gt.is_cuda or label_confusion_u8(gt, pred, num_classes, ignore_label, conf, stray) is None:
        label_confusion_aten(gt, pred, num_classes, ignore_label, conf, stray)
    if own:
        raise_on_stray(stray, num_classes, ignore_label)
        return conf
    return conf, stray


def raise_on_stray(stray, num_classes, ignore_label=255):
    s = stray.cpu().tolist()
    check_stray(int(s[0]), int(s[1]), int(num_classes), int(ignore_label))
