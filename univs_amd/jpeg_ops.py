"""Wrapper of the thirteenth header (include/univs_jpeg_hip.h): baseline JPEG frames decoded on the device.

  decode_jpegs     the files' bytes (or `jpeg_rule.Parsed`) of one video -> (uint8 [N, H, W, 3] on the device, status [N]); None when no
                   file is covered
  decode_covered   the launches alone on parsed, covered files of one geometry, with the buffers, the statuses and the rounds: tests, benches
  decode_runs      what the readers use: files in order -> runs of frames of one size on the device, a file the device does not decode
                   read by the host reader and uploaded

Flow of a call: the marker segments are walked on the host (data/jpeg_rule.parse_jpeg: no entropy byte is looked at), tables, offsets and
the entropy-coded bytes of the batch go up in ONE buffer, the four launches of csrc/jpeg_decode.hip run on the device's current stream and
`status` comes down in one copy.  A file goes to the host reader when it is not `covered` or has a non-zero status, so corrupt data
raises exactly what the host reader raises.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from .data import jpeg_rule

# include/univs_jpeg_hip.h: the bits of a file's status; -1 is this module's "not given to the device"
STATUS = {1: "offsets or restart interval", 2: "over-subscribed Huffman table", 4: "bits that are no code", 8: "zero run past the block",
          16: "data exhausted before the blocks", 32: "restart markers against the restart interval", 64: "magnitude category",
          128: "DC outside int16", 256: "outside the pinned arithmetic range", 512: "no EOI after the data"}
NOT_GIVEN = -1

# out: uint8 [N, H, W, 3]; status / rounds: int32 [N] on the host; blocks: int16 [N, blocks, 64] on the device; scratch_bytes: the device
# bytes beside the upload and `out` (compacted data, interval table, blocks, planes)
Covered = namedtuple("Covered", "out status rounds blocks scratch_bytes upload_bytes")


def status_text(s):
    if s == NOT_GIVEN:
        return "not covered"
    return ", ".join(v for k, v in STATUS.items() if s & k) or "ok"


def geometry_key(p):
    """What the files of one launch share."""
    h, v = jpeg_rule.geometry(p)[:2]
    return (p.width, p.height, len(p.components), h, v)


def _align(n, a=8):
    return -(-n // a) * a


def decode_covered(parsed, device, subseq_bits=1024, launches=None):
    """The launches on the parsed, covered files `parsed`, all of one `geometry_key`.  `launches`, a list, receives a function
    `launch(phases)` that repeats them on the buffers of this call (1: the entropy launches, 2: the pixel launches, 3: all)."""
    name = "decode_jpegs"
    device = torch.device(device)
    if device.type != "cuda":
        raise ops._cpu_refusal(name, f"device {device}")
    N = len(parsed)
    if N == 0:
        raise ValueError(f"{name}: no file")
    for i, p in enumerate(parsed):
        why = jpeg_rule.why_uncovered(p)
        if why is not None:
            raise ValueError(f"{name}: file {i} is not covered: {why}")
        if geometry_key(p) != geometry_key(parsed[0]):
            raise ValueError(f"{name}: file {i} is {geometry_key(p)}, file 0 is {geometry_key(parsed[0])}: one size and sampling per call")
    W, H, ncomp, h, v = geometry_key(parsed[0])
    _, _, mx, my, per, _ = jpeg_rule.geometry(parsed[0])
    mcus, nblocks = mx * my, mx * my * per
    huff = np.zeros((N, 6, 272), np.uint8)
    quant = np.zeros((N, 3, 64), np.uint16)
    ri = np.zeros(N, np.int32)
    soff = np.zeros(N + 1, np.int64)
    for i, p in enumerate(parsed):
        huff[i, :2 * ncomp] = jpeg_rule.table_bytes(p)
        for c in range(ncomp):
            quant[i, c] = p.quant[p.components[c][3]][1]
        ri[i] = p.restart_interval
        soff[i + 1] = soff[i] + len(p.data) - p.ecs[0]
    max_intervals = max(-(-mcus // (int(r) if 0 < r <= mcus else mcus)) for r in ri)
    src_total = int(soff[-1])
    if src_total >= 2 ** 31 or 3 * N * H * W >= 2 ** 31:
        raise ValueError(f"{name}: {src_total} source bytes and {3 * N * H * W} pixels bytes in one call, 2^31 is the bound")
    # one upload: offsets, restart intervals, tables (each part 8-byte aligned), then the entropy-coded bytes back to back
    parts = [soff.tobytes(), ri.tobytes(), huff.tobytes(), quant.tobytes()]
    starts, host = [], bytearray()
    for part in parts:
        starts.append(len(host))
        host += part
        host += bytes(_align(len(host)) - len(host))
    starts.append(len(host))
    for p in parsed:
        host += memoryview(p.data)[p.ecs[0]:]
    host += bytes(8)
    up = torch.frombuffer(host, dtype=torch.uint8).to(device)
    base = up.data_ptr()
    plane_bytes = (my * v * 8) * (mx * h * 8) + (2 * (my * 8) * (mx * 8) if ncomp == 3 else 0)
    comp = torch.empty(max(src_total, 8), dtype=torch.uint8, device=device)
    ivl = torch.empty((N, max_intervals + 1), dtype=torch.int32, device=device)
    blocks = torch.empty((N, nblocks, 64), dtype=torch.int16, device=device)
    planes = torch.empty((N, plane_bytes), dtype=torch.uint8, device=device)
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=device)
    status = torch.empty(N, dtype=torch.int32, device=device)
    rounds = torch.empty(N, dtype=torch.int32, device=device)

    def launch(phases=3):
        ops._call(name, _lib.load().univs_jpeg_decode, up, base + starts[4], base + starts[0], base + starts[1], base + starts[2],
                  base + starts[3], N, W, H, ncomp, h, v, int(subseq_bits), int(max_intervals), src_total, int(phases), ops._ptr(comp),
                  ops._ptr(ivl), ops._ptr(blocks), ops._ptr(planes), ops._ptr(out), ops._ptr(status), ops._ptr(rounds), uncovered="raise")
    launch(3)
    if launches is not None:
        launches.append(launch)
    st = torch.stack([status, rounds]).cpu().numpy()                 # (the one download; it also orders `up`'s release after the launches)
    scratch = comp.numel() + 4 * ivl.numel() + 2 * blocks.numel() + planes.numel()
    return Covered(out, st[0], st[1], blocks, scratch, len(host))


def _parsed(item):
    return item if isinstance(item, jpeg_rule.Parsed) else jpeg_rule.parse_jpeg(item)


def decode_jpegs(files, device, subseq_bits=1024):
    """(uint8 [N, H, W, 3] on `device`, int32 status [N] on the host) of N files, each bytes or a `jpeg_rule.Parsed`: the frames of one
    video.  Frame i is `np.asarray(PIL.Image.open(f).convert("RGB"))` bit for bit where status[i] == 0; a positive status is the
    device's (include/univs_jpeg_hip.h), -1 marks a file that was not given to it: not covered (`jpeg_rule.why_uncovered`), or of
    another size or sampling than the first covered file.  The pixels of such frames are unspecified.  None when no file is covered.
    A CPU `device` raises like every wrapper."""
    name = "decode_jpegs"
    device = torch.device(device)
    if device.type != "cuda":
        raise ops._cpu_refusal(name, f"device {device}")
    if int(subseq_bits) < 32 or int(subseq_bits) % 32:
        raise ValueError(f"{name}: subseq_bits={subseq_bits!r} (a multiple of 32)")
    parsed = [_parsed(f) for f in files]
    take = [i for i, p in enumerate(parsed) if jpeg_rule.covered(p)]
    if not take:
        return None
    key = geometry_key(parsed[take[0]])
    take = [i for i in take if geometry_key(parsed[i]) == key]
    res = decode_covered([parsed[i] for i in take], device, subseq_bits)
    status = np.full(len(parsed), NOT_GIVEN, np.int32)
    status[take] = res.status
    if len(take) == len(parsed):
        return res.out, status
    out = torch.zeros((len(parsed),) + tuple(res.out.shape[1:]), dtype=torch.uint8, device=device)
    out[torch.as_tensor(take, device=device)] = res.out
    return out, status


def decode_runs(datas, device, host_reader, batch_bytes=256 << 20, subseq_bits=1024, on_fallback=None):
    """The files `datas` (bytes each), in order, as a list of uint8 [n, H, W, 3] device tensors, each a run of consecutive files of
    one size: the frames the device decoded are views of the launch's output, a file it does not decode (not covered, or a non-zero
    status) is `host_reader(index)` (uint8 [H, W, 3], numpy) uploaded as a run of its own, so its errors are the host reader's.  A
    launch takes consecutive covered files of one size and sampling whose decoded frames stay within `batch_bytes`.
    `on_fallback(index, reason)` is told about every file the host read."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ops._cpu_refusal("decode_jpegs", f"device {device}")
    parsed = [jpeg_rule.parse_jpeg(d) for d in datas]
    reasons = [jpeg_rule.why_uncovered(p) for p in parsed]
    runs, i = [], 0

    def host(k, reason):
        if on_fallback is not None:
            on_fallback(k, reason)
        runs.append(torch.from_numpy(np.array(host_reader(k))).to(device)[None])   # (a copy: Pillow's arrays are read-only)

    while i < len(parsed):
        if reasons[i] is not None:
            host(i, reasons[i])
            i += 1
            continue
        key, frame_bytes = geometry_key(parsed[i]), 3 * parsed[i].width * parsed[i].height
        j = i + 1
        while j < len(parsed) and reasons[j] is None and geometry_key(parsed[j]) == key and (j - i + 1) * frame_bytes <= batch_bytes:
            j += 1
        res = decode_covered(parsed[i:j], device, subseq_bits)
        a = 0
        for b in range(j - i + 1):                                   # maximal runs of frames with status 0; the others one by one
            if b == j - i or res.status[b] != 0:
                if b > a:
                    runs.append(res.out[a:b])
                if b < j - i:
                    host(i + b, "status %d (%s)" % (res.status[b], status_text(int(res.status[b]))))
                a = b + 1
        i = j
    return runs
