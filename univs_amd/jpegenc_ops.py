"""Wrapper of the fourteenth header (include/univs_jpegenc_hip.h): baseline JPEG files encoded on the device.

  encode_jpegs     uint8 [N, H, W, 3] on the device (and optionally the result to overlay: ids, lut, edge) -> the N files' bytes
  encode_covered   the launches alone, with the buffers, the statuses and the byte counts: tests, benches

Flow of a call: the coefficient launches of csrc/jpeg_encode.hip run on the device's current stream and leave the bits of every frame;
these totals come down in one small copy and size the stream buffers (the data before stuffing, and twice that for the stuffed bytes: not
the worst case of 208 bytes a block); the stream launches pack and stuff; lengths and statuses come down, then the data in one copy.
The host prepends the marker segments (data/jpeg_encode_rule.headers: the same bytes the rule writes) and appends EOI.  What the entry
does not cover, and a frame with a non-zero status, Pillow encodes from the downloaded (and, with ids, overlaid) frame.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from .data import jpeg_encode_rule
from .inference import overlay_rule

# include/univs_jpegenc_hip.h: the bits of a frame's status
STATUS = {1: "DC category above 11", 2: "AC category above 10", 4: "stream region too small"}
_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}

# data: [bytes per frame], the entropy-coded data with the stuffing; status: int32 [N] on the host; blocks: int16 [N, B, 64] on the
# device; totals: the bits of every frame; scratch_bytes: the device bytes beside the inputs (coefficients, sizes, offsets, both stream
# buffers); stream_bytes: the bytes of the N streams
Covered = namedtuple("Covered", "data status blocks totals scratch_bytes stream_bytes")


def status_text(s):
    return ", ".join(v for k, v in STATUS.items() if s & k) or "ok"


def _check(name, rgb, quality, sampling, ids, lut, edge):
    if not isinstance(rgb, torch.Tensor) or rgb.device.type != "cuda":
        raise ops._cpu_refusal(name, f"tensor on {rgb.device}" if isinstance(rgb, torch.Tensor) else f"{type(rgb).__name__}")
    if rgb.ndim != 4 or rgb.shape[3] != 3 or rgb.dtype != torch.uint8 or rgb.shape[1] < 1 or rgb.shape[2] < 1:
        raise ValueError(f"{name}: rgb is uint8 [N, H, W, 3], got {rgb.dtype} {tuple(rgb.shape)}")
    if sampling not in jpeg_encode_rule.SAMPLINGS:
        raise ValueError(f'{name}: sampling="{sampling}": "444", "422" or "420"')
    if int(quality) != quality:
        raise ValueError(f"{name}: quality={quality!r} (an integer)")
    if (ids is None) != (lut is None):
        raise ValueError(f"{name}: ids and lut go together")
    if ids is None:
        return rgb.contiguous(), None, None, None
    if not isinstance(ids, torch.Tensor) or ids.device != rgb.device:
        raise ops._cpu_refusal(name, f"ids on {ids.device}" if isinstance(ids, torch.Tensor) else f"ids {type(ids).__name__}")
    if tuple(ids.shape) != tuple(rgb.shape[:3]) or ids.dtype.is_floating_point or ids.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"{name}: ids is an integer [N, H, W] of rgb's size, got {ids.dtype} {tuple(ids.shape)} against {tuple(rgb.shape)}")
    lut = overlay_rule.check_lut(lut.cpu().numpy() if isinstance(lut, torch.Tensor) else lut)
    if ids.dtype not in (torch.uint8, torch.int32):                  # (the clamp first: a wide id must not wrap into the table)
        ids = ids.clamp(-1, lut.shape[0]).to(torch.int32)
    return rgb.contiguous(), ids.contiguous(), lut, overlay_rule.check_edge(edge)


def encode_covered(rgb, quality=90, sampling="420", ids=None, lut=None, edge=overlay_rule.OFF_WHITE, launches=None):
    """The launches on the frames `rgb`; None where the entry does not cover the call.  `launches`, a list, receives a function
    `launch(phases)` that repeats them on the buffers of this call (1: the coefficient launches, 2: the stream launches, 3: all)."""
    name = "encode_jpegs"
    rgb, ids, lut, edge = _check(name, rgb, quality, sampling, ids, lut, edge)
    N, H, W = (int(x) for x in rgb.shape[:3])
    device = rgb.device
    h, v = jpeg_encode_rule.SAMPLINGS[sampling]
    B = (-(-W // (8 * h))) * (-(-H // (8 * v))) * (h * v + 2)
    if N == 0:
        return Covered([], np.zeros(0, np.int32), torch.empty((0, B, 64), dtype=torch.int16, device=device), np.zeros(0, np.int64), 0, 0)
    if N * B * 128 >= 2 ** 40:
        return None
    lut_d = None if lut is None else torch.from_numpy(np.ascontiguousarray(lut)).to(device)
    edge_i = -1 if edge is None else (edge[0] << 16) | (edge[1] << 8) | edge[2]
    blocks = torch.empty((N, B, 64), dtype=torch.int16, device=device)
    sizes = torch.empty((N, B), dtype=torch.int32, device=device)
    bit_off = torch.empty((N, B), dtype=torch.int64, device=device)
    totals = torch.empty(N, dtype=torch.int64, device=device)
    status = torch.empty(N, dtype=torch.int32, device=device)
    bufs = {}

    def launch(phases):
        p = {k: ops._opt(bufs.get(k)) for k in ("raw_off", "raw", "out", "out_len")}
        return ops._call(name, _lib.load().univs_jpeg_encode, rgb, ops._ptr(rgb), ops._opt(ids), int(ids is not None and ids.dtype == torch.int32),
                         ops._opt(lut_d), 0 if lut is None else int(lut.shape[0]), edge_i, N, H, W, h, v, int(quality), int(phases),
                         ops._ptr(blocks), ops._ptr(sizes), ops._ptr(bit_off), ops._ptr(totals), p["raw_off"], bufs.get("raw_total", 0),
                         p["raw"], p["out"], p["out_len"], ops._ptr(status))

    if not launch(1):
        return None
    bits = totals.cpu().numpy()                                      # (the small download that sizes the stream buffers)
    raw_off = np.zeros(N + 1, np.int64)
    raw_off[1:] = np.cumsum((((bits + 7) >> 3) + 3) & ~3)
    bufs["raw_total"] = int(raw_off[-1])
    bufs["raw_off"] = torch.from_numpy(raw_off).to(device)
    bufs["raw"] = torch.empty(max(bufs["raw_total"], 4), dtype=torch.uint8, device=device)
    bufs["out"] = torch.empty(max(2 * bufs["raw_total"], 4), dtype=torch.uint8, device=device)
    bufs["out_len"] = torch.empty(N, dtype=torch.int64, device=device)
    if not launch(2):
        return None
    if launches is not None:
        launches.append(launch)
    lens = bufs["out_len"].cpu().numpy()
    st = status.cpu().numpy()
    pieces = [bufs["out"][2 * int(raw_off[i]):2 * int(raw_off[i]) + int(lens[i])] for i in range(N)]
    flat = torch.cat(pieces).cpu().numpy().tobytes()                 # (one download for the N streams)
    ends = np.cumsum(lens)
    data = [flat[int(e - n):int(e)] for e, n in zip(ends, lens)]
    scratch = 2 * blocks.numel() + 4 * sizes.numel() + 8 * bit_off.numel() + bufs["raw"].numel() + bufs["out"].numel()
    return Covered(data, st, blocks, bits, scratch, int(lens.sum()))


def _pillow(frame, quality, sampling):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=int(quality), subsampling=_SUBSAMPLING[sampling])
    return buf.getvalue()


def encode_jpegs(rgb, quality=90, sampling="420", ids=None, lut=None, edge=overlay_rule.OFF_WHITE):
    """The bytes of N JPEG files of the frames `rgb`, uint8 [N, H, W, 3] on the device: file i is
    `Image.fromarray(frame_i).save(f, "JPEG", quality=quality, subsampling=...)` byte for byte.  With `ids` (integer [N, H, W] on the
    device) and `lut` (uint8 [K, 4]) the frames are overlaid as inference/overlay_rule.overlay_rule does, inside the encoder.  A CPU tensor
    raises like every wrapper."""
    res = encode_covered(rgb, quality, sampling, ids, lut, edge)
    N, H, W = (int(x) for x in rgb.shape[:3])
    head = jpeg_encode_rule.headers(W, H, quality, sampling) if res is not None else None
    files = []
    for i in range(N):
        if res is not None and res.status[i] == 0:
            files.append(head + res.data[i] + b"\xff\xd9")
            continue
        frame = rgb[i].cpu().numpy()                                 # not covered, or a status: the host's encoder
        if ids is not None:
            frame = overlay_rule.overlay_rule(frame, ids[i].cpu().numpy(), lut.cpu().numpy() if isinstance(lut, torch.Tensor) else lut, edge)
        files.append(_pillow(frame, quality, sampling))
    return files
