"""What the three count wrappers (pair_counts.py, vss_counts.py, davis_counts.py) and their drivers share.  A wrapper is

    admit(name, gt, pred, check, ...)     CPU refusal, then the module's own argument check, then the device mismatch: in this order
    its coverage bound -> None            the module's own (csrc/*_count.hip's), before anything is allocated
    launch(name, "univs_...", gt, outputs, ...)

and its module's `*_counts` is `kernel_else_aten`.  The kernels are csrc/pair_count.hip, vss_count.hip and davis_count.hip over
csrc/count_core.h; the contract of all three wrappers is pinned in tests/test_eval_counts_contract_cpu.py.  pvos_counts.py
(csrc/pvos_count.hip) is written over the same three steps; tests/test_pvos_eval_cpu.py pins its contract.
"""
import logging

import numpy as np
import torch

from .. import _lib, ops


def check_uint8_pair(name, gt, pred):
    """gt and pred are uint8 and cover the same non-empty [T, H, W]."""
    for side, x in (("gt", gt), ("pred", pred)):
        if x.dtype != torch.uint8 or x.dim() != 3:
            raise RuntimeError(f"{name}: {side} must be uint8 [T, H, W], got {x.dtype} {tuple(x.shape)}")
    if tuple(gt.shape) != tuple(pred.shape) or 0 in gt.shape:
        raise RuntimeError(f"{name}: gt {tuple(gt.shape)} and pred {tuple(pred.shape)} do not cover the same non-empty [T, H, W]")


def admit(name, gt, pred, check, *args):
    """The prologue of a kernel wrapper: CPU tensors raise as in every wrapper of ops.py, then `check(name, gt, pred, *args)` (whose
    result is returned), then two devices raise."""
    for side, t in (("gt", gt), ("pred", pred)):
        if not t.is_cuda:
            raise ops._cpu_refusal(name, f"{side} on {t.device}")
    r = check(name, gt, pred, *args)
    if pred.device != gt.device:
        raise RuntimeError(f"{name}: gt on {gt.device}, pred on {pred.device}")
    return r


def launch(name, fn, anchor, outputs, *args):
    """`fn` of the library (by name: looked up at call time) on `args`, then the pointers of the freshly allocated `outputs`, on
    `anchor`'s device and current stream: `outputs`, or None where the kernel does not cover the call."""
    ok = ops._call(name, getattr(_lib.load(), fn), anchor, *args, *(ops._ptr(o) for o in outputs))
    return outputs if ok else None


def kernel_else_aten(kernel, aten, gt, pred, *args):
    """The kernel on GPU tensors where it covers the call, else the ATen formulation."""
    if gt.is_cuda and pred.is_cuda:
        r = kernel(gt, pred, *args)
        if r is not None:
            return r
    return aten(gt, pred, *args)


# ---- the drivers (vss.py, davis.py) -------------------------------------------------------------------------------------------------
def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


READERS = ("host", "gpu")


def check_reader(reader):
    """`reader` of the file scorers: "host" (Pillow per file on the host, the default) or "gpu" (png_read_ops.read_pngs_device)."""
    if reader not in READERS:
        raise ValueError(f"reader={reader!r}: host or gpu")
    return reader


class _Irregular(Exception):
    pass


HOST_FALLBACKS = []           # (first path, reason) of every `device_stack` call that handed its files to the host loop


def _to_host_loop(paths, reason):
    """reader "gpu" is leaving these files to Pillow: said in the log and counted in HOST_FALLBACKS, so that a data set whose videos all
    hold one file the device does not take is not scored by the host without a sign."""
    HOST_FALLBACKS.append((paths[0], reason))
    logging.getLogger(__name__).warning("reader=gpu: the %d files from %s on are read by the host loop: %s", len(paths), paths[0], reason)
    return None


def device_stack(paths, reader="host", device=None, rgb=False):
    """The one switch between the two readers.  reader "host": None, and the caller runs its own Pillow loop, today's code path.
    reader "gpu": the PNG files `paths` decoded on the device by ONE `read_pngs_device` call and stacked there, uint8 [T, H, W] (rgb:
    [T, H, W, 3], as `.convert("RGB")`); no plane is copied to the host.  None also where the files are not regular: one of them is
    missing, is not decoded by the device (it does not parse, is not covered, breaks a rule of its stream), is no [H, W] plane, or has
    another size than the first.  The caller's host loop then meets that file in its own order and raises what it raises today; the
    hand-over is logged as a warning and recorded in HOST_FALLBACKS."""
    check_reader(reader)
    if reader == "host" or not paths:
        return None
    from .. import png_read_ops

    def irregular(index):
        raise _Irregular(index)
    try:
        datas = []
        for p in paths:
            with open(p, "rb") as f:
                datas.append(f.read())
        planes = png_read_ops.read_pngs_device(datas, pick_device(device), rgb=rgb, host_reader=irregular)
    except OSError as e:
        return _to_host_loop(paths, f"{type(e).__name__}: {e}")
    except _Irregular as e:
        return _to_host_loop(paths, f"{paths[e.args[0]]} is not decoded by the device (it does not parse, is not covered, or breaks a rule)")
    if any(p.dim() != (3 if rgb else 2) or p.shape != planes[0].shape for p in planes):
        return _to_host_loop(paths, "the files are not planes of one size")
    return torch.stack(planes)


def stack(planes):
    """np.stack, or torch.stack for device planes."""
    return torch.stack(list(planes)) if isinstance(planes[0], torch.Tensor) else np.stack(planes)


def pick_device(device, like=None):
    """`device` when it is given, else the device of the GPU tensor `like`, else the GPU when there is one."""
    if device is not None:
        return torch.device(device)
    if like is not None and like.is_cuda:
        return like.device
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")
