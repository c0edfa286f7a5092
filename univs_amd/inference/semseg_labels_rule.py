"""The two rules of include/univs_imagelabels_hip.h in numpy: the yardstick of csrc/semseg_labels.hip on the CPU.

  semseg_labels_rule     labels[y, x] = argmax_c bilinear(r_c -> H x W)(y, x), the first maximum winning
  label_confusion_rule   conf[(K + 1), (K + 1)] += 1 per pixel, row = ground truth (ignore_label -> K), column = prediction

The resize is stated in float32 with ATen's source-index expression (UpSampleBilinear2d: `area_pixel_compute_source_index` without
align_corners, the scale in / out as a float32 quotient, the weights l1 = src - i0, l0 = 1 - l1) and the blend of csrc/resample_taps.h
(`bilerp`: two products, then three fused multiply-adds).  numpy has no fused multiply-add, so the blend is evaluated in float64 and
rounded once per fma: a float32 product is exact in float64, and the double rounding that remains can differ from the device's single
rounding in the last bit only.  The argmax of the device and this rule therefore agree wherever the two largest values differ by more
than a rounding; the tie rule itself (strict > while c ascends) is exact here and is tested on planes where the compared values are
equal bit for bit.
"""
import numpy as np

F32 = np.float32


def taps(in_size, out_size):
    """(i0 int64 [out], i1 int64 [out], l0 float32 [out], l1 float32 [out]) of ATen's bilinear resize along one axis."""
    scale = F32(in_size) / F32(out_size)
    dst = np.arange(out_size, dtype=F32)
    src = scale * (dst + F32(0.5)) - F32(0.5)
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    l0 = (F32(1) - l1).astype(F32)
    return i0, i1, l0, l1


def _fma(a, b, c):
    """round_f32(a b + c) for float32 a, b, c, through float64 (a b is exact there)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def resized_plane(plane, out_size):
    """bilinear(plane [hi, wi] -> out_size) in float32: csrc/resample_taps.h's `bilerp` on ATen's taps."""
    plane = np.asarray(plane, dtype=F32)
    y0, y1, ly0, ly1 = taps(plane.shape[0], out_size[0])
    x0, x1, lx0, lx1 = taps(plane.shape[1], out_size[1])
    a, b = plane[y0][:, x0], plane[y0][:, x1]
    c, d = plane[y1][:, x0], plane[y1][:, x1]
    top = _fma(lx1[None], b, (lx0[None] * a).astype(F32))
    bot = _fma(lx1[None], d, (lx0[None] * c).astype(F32))
    return _fma(ly1[:, None], bot, (ly0[:, None] * top).astype(F32))


def semseg_labels_rule(r, out_size):
    """uint8 [H, W]: the class whose resized plane is largest; strict > while c ascends, so the first maximum wins.  r: [C, hi, wi],
    1 <= C <= 256."""
    r = np.asarray(r, dtype=F32)
    if r.ndim != 3 or not 1 <= r.shape[0] <= 256:
        raise ValueError(f"semseg_labels_rule: float32 [C, hi, wi] with 1 <= C <= 256, got {r.shape}")
    best = resized_plane(r[0], out_size)
    labels = np.zeros(best.shape, dtype=np.uint8)
    for c in range(1, r.shape[0]):
        u = resized_plane(r[c], out_size)
        win = u > best
        best = np.where(win, u, best)
        labels[win] = c
    return labels


def label_confusion_rule(gt, pred, num_classes, ignore_label=255):
    """int64 [(K + 1), (K + 1)] of two uint8 maps of one shape: row = ground truth with ignore_label -> K, column = prediction.  A
    ground-truth value that is neither < K nor the ignore label, or a prediction > K, is a ValueError (the wrapper's, from the
    kernel's stray counts)."""
    K = int(num_classes)
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    if g.shape != p.shape:
        raise ValueError(f"label_confusion: {g.size} ground-truth and {p.size} predicted pixels")
    row = np.where(g == ignore_label, K, g)
    check_stray(int(((row > K) | ((row == K) & (g != ignore_label))).sum()), int((p > K).sum()), K, ignore_label)
    return np.bincount((K + 1) * row + p, minlength=(K + 1) ** 2).reshape(K + 1, K + 1)


def check_stray(stray_gt, stray_pred, num_classes, ignore_label):
    if stray_gt:
        raise ValueError(f"label_confusion: {stray_gt} ground-truth pixels are neither a class below {num_classes} nor the ignore label "
                         f"{ignore_label}")
    if stray_pred:
        raise ValueError(f"label_confusion: {stray_pred} predicted pixels are above {num_classes}")
