"""The counts of a VIPOSeg panoptic-VOS evaluation, per video: everything the mask IoU and the boundary IoU of every tracked id need
(pvos.py).

  pvos_video_counts   the HIP kernel (csrc/pvos_count.hip) behind `ops._call`: GPU tensors only, None where it does not cover
  pvos_counts_aten    the same tensor from torch ops on any device: the fallback, the yardstick, the CPU path
  pvos_counts         the kernel on GPU tensors where it covers the call, else the ATen formulation
  dilation            the d of a frame size (eval_utils_viposeg.py:34-38)

gt is uint8 [T, H, W], the raw bytes of the annotation PNGs, pred uint8 [T, H, W], the bytes of the result PNGs.  All three return
int32 [T, K, 6]; cell [t, k - 1] = (I, A_g, A_p, BI, B_g, B_p) of id k in frame t:

  I, A_g, A_p      pixels with gt == pred == k, with gt == k, with pred == k
  B_g, B_p         boundary pixels of id k in the gt, in the result: what `mask_to_boundary` leaves of the id's mask, i.e.
                   mask - erode(copyMakeBorder(mask, 1 pixel of 0), 3 x 3 ones, iterations=d)
  BI               pixels with gt == pred == k that are boundary on both sides

A label map gives each pixel to one id, so a pixel is a boundary pixel of ITS id exactly when the (2 d + 1) x (2 d + 1) window around
it holds another label or leaves the image: one pass serves every id.  Ids 0 and above K are not counted, but they are labels like any
other where a window's uniformity is decided.
"""
import numpy as np
import torch

from .. import ops
from . import _counts

D_MAX = 88            # csrc/pvos_count.hip: PV_D_MAX, the halo in LDS (the d of a 4K frame)
K_MAX = 255           # PV_K_MAX: an id is a byte


def dilation(H, W, ratio=0.02):
    """The number of 3 x 3 erosions of `mask_to_boundary`: round(ratio * diagonal), at least 1.  29 at 720 x 1280, 44 at 1080 x 1920."""
    return max(1, int(round(ratio * np.sqrt(H ** 2 + W ** 2))))


def _check(name, gt, pred, d, K):
    _counts.check_uint8_pair(name, gt, pred)
    if int(d) != d or int(d) < 1:
        raise RuntimeError(f"{name}: d {d}")
    if int(K) != K or int(K) < 1:
        raise RuntimeError(f"{name}: largest id K={K}")


def pvos_video_counts(gt, pred, d, K):
    """counts int32 [T, K, 6] from csrc/pvos_count.hip on the tensors' device and current stream; None where the kernel does not cover
    the call (d > D_MAX, K > K_MAX, T H W >= 2^31): the caller keeps `pvos_counts_aten`.  CPU tensors raise, as in every wrapper of
    ops.py."""
    name = "pvos_video_counts"
    _counts.admit(name, gt, pred, _check, d, K)
    T, H, W = (int(v) for v in gt.shape)
    d, K = int(d), int(K)
    if d > D_MAX or K > K_MAX or T * H * W >= 2 ** 31:
        return None
    gt, pred = gt.contiguous(), pred.contiguous()
    out = _counts.launch(name, "univs_pvos_counts", gt, (torch.zeros((T, K, 6), dtype=torch.int32, device=gt.device),), ops._ptr(gt),
                         ops._ptr(pred), T, H, W, d, K)
    return None if out is None else out[0]


def window_not_uniform(x, d):
    """bool [H, W]: the (2 d + 1)^2 window around the pixel of the uint8 map `x` holds two labels or leaves the image.  The map is
    padded with -1 by d; the window's maximum and minimum (each a row pool, then a column pool) differ exactly there."""
    H, W = x.shape
    p = torch.nn.functional.pad(x.to(torch.float32)[None, None], (d, d, d, d), value=-1.0)      # (labels <= 255: exact)

    def pool(v):
        v = torch.nn.functional.max_pool2d(v, (1, 2 * d + 1), stride=1)
        return torch.nn.functional.max_pool2d(v, (2 * d + 1, 1), stride=1)
    return (pool(p) != -pool(-p)).reshape(H, W)


def pvos_counts_aten(gt, pred, d, K):
    """counts int32 [T, K, 6] on the tensors' device, CPU or GPU: per frame, the two boundary maps from a max-pool and a min-pool of
    window 2 d + 1 over the map padded with -1, then three `bincount`s of (label, boundary) cells.  Exact."""
    _check("pvos_counts_aten", gt, pred, d, K)
    d, K = int(d), int(K)
    T = int(gt.shape[0])
    dev = gt.device
    pred = pred.to(dev)
    out = torch.zeros((T, K, 6), dtype=torch.int32, device=dev)
    n = min(K, 255)
    for t in range(T):
        g, p = gt[t], pred[t]
        bg, bp = window_not_uniform(g, d), window_not_uniform(p, d)
        gl, pl = g.reshape(-1).to(torch.int64), p.reshape(-1).to(torch.int64)
        cg = torch.bincount(gl * 2 + bg.reshape(-1), minlength=512).reshape(256, 2)
        cp = torch.bincount(pl * 2 + bp.reshape(-1), minlength=512).reshape(256, 2)
        eq = gl == pl
        ci = torch.bincount(gl[eq] * 2 + (bg & bp).reshape(-1)[eq], minlength=512).reshape(256, 2)
        cells = torch.stack([ci.sum(dim=1), cg.sum(dim=1), cp.sum(dim=1), ci[:, 1], cg[:, 1], cp[:, 1]], dim=1)
        out[t, :n] = cells[1:n + 1].to(torch.int32)
    return out


def pvos_counts(gt, pred, d, K):
    """counts int32 [T, K, 6]: the kernel on GPU tensors where it covers the call, else the ATen formulation."""
    return _counts.kernel_else_aten(pvos_video_counts, pvos_counts_aten, gt, pred, d, K)
