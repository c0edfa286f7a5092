"""Wrapper of the tenth header (include/univs_png_hip.h): result PNGs whose zlib streams the device encodes.

  deflate_maps   the HIP kernels (csrc/png_deflate.hip) behind `ops._call`: GPU tensors only (a CPU tensor raises), None where the
                 kernels do not cover the call; deflate_maps_device is the same call without the downloads
  png_files      the files around the streams, through the chunk writer of inference/png_rule.py

src is a stack of id maps [N, H, W], uint8 or int32; lut uint8 [K, channels] gives the pixel bytes lut[clamp(id, 0, K - 1)] (None:
the ids themselves, uint8 and one channel).  The result is one zlib stream per frame, as `bytes` on the host: inference/png_rule.py
states them byte for byte and is the yardstick.  Two device-to-host copies are made: the offsets, then the used part of the output.
"""
import torch

from . import _lib, ops
from .inference import png_rule


def deflate_maps_device(src, lut=None, channels=1):
    """(out uint8, offsets int64 [N + 1]) on the device: stream f is out[offsets[f] : offsets[f + 1]], nothing is downloaded.  None where
    the kernels do not cover the sizes; CPU tensors raise.  `deflate_maps` is this and the two downloads."""
    name = "deflate_maps"
    ops._require_gpu(name, src, *(() if lut is None else (lut,)))
    C = int(channels)
    if src.dtype not in (torch.uint8, torch.int32) or src.dim() != 3:
        raise RuntimeError(f"{name}: uint8 or int32 id maps [N, H, W], got {src.dtype} {tuple(src.shape)}")
    if C not in (1, 3):
        raise RuntimeError(f"{name}: channels {channels}")
    if lut is None:
        if src.dtype != torch.uint8 or C != 1:
            raise RuntimeError(f"{name}: without a lut the ids are the pixels: uint8 and one channel, got {src.dtype} and {C}")
    elif lut.dtype != torch.uint8 or lut.dim() != 2 or lut.shape[1] != C or lut.shape[0] < 1 or lut.device != src.device:
        raise RuntimeError(f"{name}: lut uint8 [K, {C}] on {src.device}, got {lut.dtype} {tuple(lut.shape)} on {lut.device}")
    N, H, W = (int(v) for v in src.shape)
    if N and (H < 1 or W < 1):
        raise RuntimeError(f"{name}: empty frames {tuple(src.shape)}")
    if N == 0:
        return torch.empty(0, dtype=torch.uint8, device=src.device), torch.zeros(1, dtype=torch.int64, device=src.device)
    row_len = W * C + 1
    R = png_rule.stripe_rows(row_len)
    if R is None or N * H * row_len >= 2 ** 31:
        return None                                                  # (the entry's answer, without buffers it would not fill)
    S = -(-H // R)
    scratch = torch.empty(png_rule.scratch_bytes(N, H, row_len), dtype=torch.uint8, device=src.device)
    out = torch.empty(N * (8 + S * png_rule.stripe_capacity(R * row_len)), dtype=torch.uint8, device=src.device)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=src.device)
    ok = ops._call(name, _lib.load().univs_png_deflate_maps, src, ops._ptr(src), int(src.dtype == torch.int32), N, H, W, ops._opt(lut),
                   1 if lut is None else int(lut.shape[0]), C, R, ops._ptr(scratch), ops._ptr(out), ops._ptr(offsets))
    return (out, offsets) if ok else None


def deflate_maps(src, lut=None, channels=1):
    """list of N `bytes` from csrc/png_deflate.hip on src's device and current stream.  None where the kernels do not cover the sizes
    (include/univs_png_hip.h states them: a row beyond the stripe cap, or 2^31 filtered bytes): the caller saves with Pillow.  CPU
    tensors raise, as in every wrapper of ops.py."""
    res = deflate_maps_device(src, lut, channels)
    if res is None:
        return None
    out, offsets = res
    ends = offsets.cpu().tolist()
    data = out[:ends[-1]].cpu().numpy().tobytes()
    return [data[ends[i]:ends[i + 1]] for i in range(len(ends) - 1)]


def png_files(streams, H, W, channels=1, palette=None):
    """The PNG file of every stream: signature, IHDR, PLTE when a palette is given, one IDAT, IEND."""
    return [png_rule.png_file(s, H, W, channels, palette) for s in streams]
