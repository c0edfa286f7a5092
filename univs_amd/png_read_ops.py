"""Wrapper of the twelfth header (include/univs_pngread_hip.h): PNG files decoded on the device.

  read_pngs_device   the files' bytes -> one uint8 device tensor per file, what `np.array(PIL.Image.open(...))` returns (rgb=True:
                     of `.convert("RGB")`); a file the kernels do not take goes through Pillow on the host, on its own
  read_covered       the launches alone on parsed files (inference/png_read.py), with the buffers and the statuses: tests and benches

Flow of a call: the containers are parsed on the host, the zlib streams and the small tables go up in ONE buffer, the two launches of
csrc/png_inflate.hip run on the device's current stream, and `status` comes down in one copy.  A file falls back to the host reader
when it does not parse, is not `covered`, or has a non-zero status: corrupt data raises exactly what the host reader raises.
"""
import io
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from .inference import png_read

# csrc/png_inflate_core.h: PngStatus
STATUS = {0: "ok", 1: "descriptor or offsets", 2: "zlib header", 3: "input exhausted", 4: "block type 3", 5: "stored block LEN / NLEN",
          6: "over-subscribed or incomplete code", 7: "repeat code without a previous length", 8: "invalid symbol or distance code",
          9: "distance beyond the bytes produced", 10: "more bytes than the image has", 11: "fewer bytes than the image has", 12: "Adler-32",
          13: "filter byte above 4"}

# planes: the N tensors (views of `out`); status: int32 [N] on the host; filtered / out: the device buffers with their margins;
# filt_offsets / out_offsets: [N + 1] on the host, relative to the buffers' starts (margins included); filt_sizes / out_sizes: the bytes
# each file has in them
Covered = namedtuple("Covered", "planes status filtered out filt_offsets out_offsets filt_sizes out_sizes")


class UncoveredPng(RuntimeError):
    pass


def _out_channels(info, rgb):
    return 3 if (rgb or info.colour_type == 2) else 1


def _align(n, a=8):
    return -(-n // a) * a


def read_covered(infos, device, rgb=False, margin=0, gap=0, marker=0, launches=None):
    """The two launches on the parsed, covered files `infos`.  `margin` bytes before and after the filtered and the output buffer and
    `gap` bytes after every file's region are filled with `marker` and belong to no file: the kernels must leave them alone.  `launches`, a
    list, receives a function that repeats the two launches on the buffers of this call."""
    name = "read_pngs_device"
    device = torch.device(device)
    if device.type != "cuda":
        raise ops._cpu_refusal(name, f"device {device}")
    N = len(infos)
    for i, info in enumerate(infos):
        if not png_read.covered(info):
            raise UncoveredPng(f"{name}: file {i} is not covered: {png_read.why_uncovered(info)}")
    palettes = [i for i, info in enumerate(infos) if info.colour_type == 3 and rgb]
    prow = {i: k for k, i in enumerate(palettes)}
    desc = np.zeros((N, 8), np.int32)
    soff, foff, ooff = np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64), np.zeros(N + 1, np.int64)
    fsize, osize = np.zeros(N, np.int64), np.zeros(N, np.int64)
    foff[0] = ooff[0] = margin
    for i, info in enumerate(infos):
        och = _out_channels(info, rgb)
        desc[i, :6] = (info.width, info.height, info.colour_type, info.bit_depth, och, prow.get(i, 0))
        fsize[i] = info.height * (1 + png_read.rowbytes(info))
        osize[i] = info.height * info.width * och
        soff[i + 1] = soff[i] + len(info.idat)
        foff[i + 1] = foff[i] + fsize[i] + gap
        ooff[i + 1] = ooff[i] + osize[i] + gap
    filt_total, out_total = int(foff[-1]) + margin, int(ooff[-1]) + margin
    max_rb = max((png_read.rowbytes(info) for info in infos), default=1)
    if N == 0:
        empty = torch.empty(0, dtype=torch.uint8, device=device)
        return Covered([], np.zeros(0, np.int32), empty, empty, foff, ooff, fsize, osize)
    if max(filt_total, out_total, int(soff[-1])) >= 2 ** 31:
        raise UncoveredPng(f"{name}: {filt_total} filtered, {out_total} output and {int(soff[-1])} stream bytes in one call, 2^31 is the bound")
    pal = np.zeros((len(palettes), 256, 3), np.uint8)
    for k, i in enumerate(palettes):
        p = np.frombuffer(infos[i].palette, np.uint8).reshape(-1, 3)
        pal[k, :len(p)] = p                                         # a missing entry is black
    # one upload: the three offset tables, the descriptors, the palettes, the streams (each part 8-byte aligned)
    parts = [soff.tobytes(), foff.tobytes(), ooff.tobytes(), desc.tobytes(), pal.tobytes(), b"".join(info.idat for info in infos)]
    starts, host = [], bytearray()
    for part in parts:
        starts.append(len(host))
        host += part
        host += bytes(_align(len(host)) - len(host))
    host += bytes(8)                                                # (never an empty buffer)
    up = torch.frombuffer(host, dtype=torch.uint8).to(device)
    base = up.data_ptr()
    filtered = torch.full((filt_total,), marker, dtype=torch.uint8, device=device) if (margin or gap) else \
        torch.empty(filt_total, dtype=torch.uint8, device=device)
    out = torch.full((out_total,), marker, dtype=torch.uint8, device=device) if (margin or gap) else \
        torch.empty(out_total, dtype=torch.uint8, device=device)
    status = torch.empty(N, dtype=torch.int32, device=device)

    def launch():
        ops._call(name, _lib.load().univs_png_read, up, base + starts[5], base + starts[0], base + starts[3],
                  base + starts[4] if palettes else None, len(palettes), base + starts[1], base + starts[2], N, int(soff[-1]), filt_total,
                  out_total, int(max_rb), ops._ptr(filtered), ops._ptr(out), ops._ptr(status), uncovered="raise")
    launch()
    if launches is not None:
        launches.append(launch)                                     # (tools/png_read_bench.py times the two launches alone)
    st = status.cpu().numpy()                                       # (the one download; it also orders `up`'s release after the launches)
    planes = []
    for i, info in enumerate(infos):
        och = _out_channels(info, rgb)
        shape = (info.height, info.width) if och == 1 else (info.height, info.width, 3)
        planes.append(out[int(ooff[i]):int(ooff[i]) + int(osize[i])].view(shape))
    return Covered(planes, st, filtered, out, foff, ooff, fsize, osize)


def pillow_read(data, rgb=False):
    """The host reader on a file's bytes: `np.array(PIL.Image.open(...))`, of `.convert("RGB")` with rgb."""
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB") if rgb else im)


def read_pngs_device(datas, device, rgb=False, uncovered="host", host_reader=None):
    """One device tensor per PNG file in `datas` (bytes each): uint8 [H, W] (palette indices, grey) or [H, W, 3] (RGB), as
    `np.array(PIL.Image.open(f))` gives them; with rgb=True every file comes as [H, W, 3], as `.convert("RGB")` gives it.  The tensors
    of the files the device decoded are views of one buffer.

    A file that does not parse, is not covered (inference/png_read.covered) or whose stream breaks a rule (status != 0) is read by
    `host_reader(index)` (default: Pillow on the file's bytes) and uploaded on its own, so its errors are the host reader's;
    uncovered="raise" makes that an `UncoveredPng` naming the file index and the reason instead.  A CPU `device` raises like every
    wrapper; an empty list is [] without a launch."""
    name = "read_pngs_device"
    if uncovered not in ("host", "raise"):
        raise ValueError(f"{name}: uncovered={uncovered!r} (host or raise)")
    device = torch.device(device)
    if device.type != "cuda":
        raise ops._cpu_refusal(name, f"device {device}")
    datas = list(datas)
    if not datas:
        return []
    reasons, infos, where = {}, [], []
    for i, data in enumerate(datas):
        try:
            info = png_read.parse_png(data)
        except png_read.PngParseError as e:
            reasons[i] = f"does not parse: {e}"
            continue
        if not png_read.covered(info):
            reasons[i] = f"is not covered: {png_read.why_uncovered(info)}"
            continue
        infos.append(info)
        where.append(i)
    planes = [None] * len(datas)
    if infos:
        res = read_covered(infos, device, rgb)
        for k, i in enumerate(where):
            if res.status[k] == 0:
                planes[i] = res.planes[k]
            else:
                reasons[i] = f"has status {int(res.status[k])} ({STATUS.get(int(res.status[k]), 'unknown')})"
    for i in sorted(reasons):
        if uncovered == "raise":
            raise UncoveredPng(f"{name}: file {i} {reasons[i]}")
        a = host_reader(i) if host_reader is not None else pillow_read(datas[i], rgb)
        planes[i] = torch.as_tensor(np.ascontiguousarray(a)).to(device)
    return planes
