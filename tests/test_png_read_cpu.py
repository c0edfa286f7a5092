"""CPU: the host half of the device PNG reader.  The container parser (univs_amd/inference/png_read.py) against Pillow on the corpus of
tests/png_read_cases.py; the conditions the corpus has to meet, asserted; the serial decode text of the kernel
(csrc/png_inflate_core.h) compiled for the host by tools/png_inflate_host.cpp, plain and with the address and undefined-behaviour
sanitizers, over every good and every malformed stream; and the scorers' `reader` argument, whose default changes nothing."""
import inspect
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import davis_eval_cases, png_read_cases as cases, pvos_eval_cases, vps_eval_cases, vss_eval_cases
from univs_amd.evaluation import _counts, davis, pvos, vps, vss
from univs_amd.inference import png_read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = {0: 1, 2: 3, 3: 1}


def _expect(data):
    (W, H, depth, colour, *_), _, _ = cases.idat_of(data)
    return H * (1 + (W * BITS[colour] * depth + 7) // 8)


# ---- the container ------------------------------------------------------------------------------------------------------------------
def test_parse_png_against_pillow_on_the_good_corpus():
    from PIL import Image
    modes = {(0, 8): "L", (2, 8): "RGB", (3, 1): "P", (3, 2): "P", (3, 4): "P", (3, 8): "P"}
    for c in cases.good_cases():
        info = png_read.parse_png(c.data)
        with Image.open(io.BytesIO(c.data)) as im:
            assert (info.width, info.height) == im.size and modes[(info.colour_type, info.bit_depth)] == im.mode, c.name
            if im.mode == "P":
                assert list(info.palette) == im.getpalette(), c.name
            else:
                assert info.palette is None
        assert png_read.covered(info), c.name
        assert info.idat == cases.idat_of(c.data)[1]
        assert len(zlib.decompress(info.idat)) == info.height * (1 + png_read.rowbytes(info)) == len(c.filtered) == _expect(c.data), c.name
        # inside the limits of include/univs_pngread_hip.h
        assert png_read.rowbytes(info) <= png_read.MAX_ROWBYTES == 24576 and info.width >= 1 and info.height >= 1
    assert png_read.MAX_ROWBYTES >= 3 * 8191                         # the encoder's own cap fits


def test_uncovered_kinds_parse_and_are_not_covered():
    reasons = {}
    for kind, data in cases.uncovered_files().items():
        info = png_read.parse_png(data)
        assert not png_read.covered(info), kind
        reasons[kind] = png_read.why_uncovered(info)
    assert reasons == {"16-bit": "colour type 0 at bit depth 16", "LA": "colour type 4 at bit depth 8", "RGBA": "colour type 6 at bit depth 8",
                       "1-bit grey": "colour type 0 at bit depth 1", "2-bit grey": "colour type 0 at bit depth 2", "interlaced": "interlaced"}
    good = png_read.parse_png(cases.good_cases()[0].data)
    assert not png_read.covered(good._replace(compression=1)) and not png_read.covered(good._replace(filter_method=1))
    assert not png_read.covered(good._replace(colour_type=2, width=8193))          # a row beyond the cap
    assert png_read.covered(good._replace(colour_type=2, bit_depth=8, width=8191))
    assert not png_read.covered(good._replace(width=0)) and not png_read.covered(good._replace(height=2 ** 31 - 1, width=20000))


def test_a_trns_chunk_is_ignored():
    from PIL import Image
    im = Image.fromarray(cases.blobs(9, 14, 4, 1))
    im.putpalette(list(cases.palette_of(4)))
    buf = io.BytesIO()
    im.save(buf, format="PNG", transparency=2)
    assert b"tRNS" in buf.getvalue()
    info = png_read.parse_png(buf.getvalue())
    assert png_read.covered(info) and (info.colour_type, info.bit_depth) == (3, 2)


def _rechunk(data, edit):
    """The file with its chunk list [(kind, payload)] passed through `edit`."""
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        chunks.append((kind, data[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return data[:8] + b"".join(cases.chunk(k, p) for k, p in edit(chunks))


def test_parse_errors():
    good = next(c for c in cases.good_cases() if c.name.startswith("p16_")).data
    bad = {
        "signature": b"\x89PNX" + good[4:],
        "crc": good[:20] + bytes([good[20] ^ 1]) + good[21:],                              # inside IHDR
        "no IHDR": _rechunk(good, lambda ch: [c for c in ch if c[0] != b"IHDR"]),
        "no IDAT": _rechunk(good, lambda ch: [c for c in ch if c[0] != b"IDAT"]),
        "no IEND": _rechunk(good, lambda ch: [c for c in ch if c[0] != b"IEND"]),
        "no PLTE": _rechunk(good, lambda ch: [c for c in ch if c[0] != b"PLTE"]),
        "truncated": good[:len(good) - 15],
        "empty": b"",
    }
    for kind, data in bad.items():
        with pytest.raises(png_read.PngParseError):
            png_read.parse_png(data)
    # the CRC of an ancillary chunk is not looked at
    text = _rechunk(good, lambda ch: ch[:1] + [(b"tEXt", b"k\0v")] + ch[1:])
    i = text.index(b"tEXt") + 4 + 3
    assert png_read.parse_png(text[:i] + bytes([text[i] ^ 1]) + text[i + 1:]).idat == png_read.parse_png(good).idat


# ---- the corpus's own conditions ------------------------------------------------------------------------------------------------------
def _block_types(stream, limit=200000):
    """The block types of a zlib stream, in order, by a plain bit-by-bit inflate that keeps no output."""
    data, pos = stream[2:], 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((data[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def table(lengths):
        return {(code, n): s for s, (code, n) in cases.canonical(lengths).items()}

    def symbol(t):
        code, n = 0, 0
        while True:
            code, n = (code << 1) | bits(1), n + 1
            if (code, n) in t:
                return t[(code, n)]
            assert n < 16

    types = []
    while True:
        final, kind = bits(1), bits(2)
        types.append(kind)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            pos += 16 + 8 * n
        else:
            if kind == 1:
                lit, dist = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 30)
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for s in cases.CL_ORDER[:hclen]:
                    cl[s] = bits(3)
                cl, lens = table(cl), []
                while len(lens) < hlit + hdist:
                    s = symbol(cl)
                    lens += [s] if s < 16 else ([lens[-1]] * (3 + bits(2)) if s == 16 else [0] * (3 + bits(3) if s == 17 else 11 + bits(7)))
                lit, dist = table(lens[:hlit]), table(lens[hlit:])
            while True:
                s = symbol(lit)
                if s == 256:
                    break
                if s > 256:
                    bits(cases.LENGTH_EXTRA[s - 257])
                    bits(cases.DIST_EXTRA[symbol(dist)])
        assert pos < 8 * limit
        if final:
            return types


def test_the_corpus_meets_its_conditions():
    good = cases.good_cases()
    assert {c.group for c in good} == {"pillow", "filtered", "writer", "rule"} and len(cases.bad_cases()) >= 20
    heads, first, sizes, depths = [0] * 5, [0] * 5, set(), set()
    for c in good:
        info = png_read.parse_png(c.data)
        step = 1 + png_read.rowbytes(info)
        types = c.filtered[::step]
        assert len(types) == info.height
        if c.group != "writer":                                      # (the writer's bytes are 0 .. 4 everywhere)
            for t in types:
                heads[t] += 1
            first[types[0]] += 1
        if c.group == "pillow":
            sizes.add((info.width, info.height))
        depths.add((info.colour_type, info.bit_depth))
    assert min(heads) >= 32 and min(first) >= 1, (heads, first)
    assert {w for w, _ in sizes} >= set(cases.WIDTHS) and {h for _, h in sizes} >= set(cases.HEIGHTS)
    assert depths == {(0, 8), (2, 8), (3, 1), (3, 2), (3, 4), (3, 8)}
    assert any(w % 2 and d < 8 for c in good for (w, d) in [(png_read.parse_png(c.data).width, png_read.parse_png(c.data).bit_depth)])
    # block types, block counts, IDAT splits
    seen, most = set(), 0
    for c in good:
        _, idat, parts = cases.idat_of(c.data)
        if len(idat) < 1500 or "level0" in c.name:
            types = _block_types(idat)
            seen |= set(types)
            most = max(most, len(types))
    assert seen == {0, 1, 2} and most >= 3
    assert any(cases.idat_of(c.data)[2][0] == 1 for c in good)       # a split inside the two header bytes
    assert any(0 < cases.idat_of(c.data)[2][-1] < 4 for c in good)   # ... and inside the Adler-32
    big = next(c for c in good if c.name == "l_300x230_level0")
    assert len(big.filtered) >= 66000 and _block_types(cases.idat_of(big.data)[1]).count(0) >= 2
    for c in good:
        if c.group == "writer":
            assert zlib.decompress(cases.idat_of(c.data)[1]) == c.filtered
    for c in cases.bad_cases():
        assert c.zlib_ok == (c.name in ("more_bytes_than_the_image", "fewer_bytes_than_the_image", "filter_byte_5")), c.name


# ---- the decode core on the host, plain and under the sanitizers ----------------------------------------------------------------------
def _compiler():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return [shutil.which(c)]
    from univs_amd import build
    return [build._hipcc(), "-x", "c++"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("png_inflate_host") / request.param)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    cc = _compiler()
    if flags and "clang" not in subprocess.run([cc[0], "--version"], capture_output=True, text=True).stdout:
        flags += ["-static-libasan", "-static-libubsan"]            # (clang's default; the program then needs nothing from its environment)
    if "hipcc" in cc[0] and flags:
        flags = [a for f in flags for a in ("-Xarch_host", f)]
    subprocess.run([*cc, "-O1", "-g", "-std=c++17", *flags, os.path.join(ROOT, "tools", "png_inflate_host.cpp"), "-o", out], check=True)
    return out


def _fnv(data):
    h = 1469598103934665603
    for x in data:
        h = ((h ^ x) * 1099511628211) & (2 ** 64 - 1)
    return h


def _run(program, streams):
    """[(status, produced, digest)] of [(expect, stream)] through one plain subprocess of the program, in the environment as it is: the
    sanitizers' runtimes are linked into the program."""
    records = b"".join(struct.pack("<QQ", e, len(s)) + s for e, s in streams)
    r = subprocess.run([program, "-"], input=records, capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(streams)
    return [(int(a), int(b), int(c, 16)) for a, b, c in (line.split() for line in lines)]


def test_every_good_stream_inflates_to_zlibs_bytes(host_program):
    good = cases.good_cases()
    got = _run(host_program, [(len(c.filtered), cases.idat_of(c.data)[1]) for c in good])
    for c, (status, produced, digest) in zip(good, got):
        assert (status, produced) == (0, len(c.filtered)) and digest == _fnv(c.filtered), c.name


def test_every_malformed_stream_ends_with_its_status_inside_its_bounds(host_program):
    bad = cases.bad_cases()
    assert [c.name for c in cases.host_checked_bad_cases()] == [c.name for c in bad]     # what the GPU test takes is what is asserted here
    got = _run(host_program, [(_expect(c.data), cases.idat_of(c.data)[1]) for c in bad])
    for c, (status, produced, _) in zip(bad, got):
        assert status == c.status and produced <= _expect(c.data), (c.name, status, produced)
        assert (status != 0) == (c.name != "filter_byte_5")
    # every prefix of a good stream: input exhausted, never a byte too many
    c = next(c for c in cases.good_cases() if c.name == "cycle_bpp3_l6_default")
    idat = cases.idat_of(c.data)[1]
    got = _run(host_program, [(len(c.filtered), idat[:n]) for n in range(len(idat))])
    assert all(status == 3 and produced <= len(c.filtered) for status, produced, _ in got)
    # every single-byte corruption of a small stream ends, with any status, inside the output
    got = _run(host_program, [(len(c.filtered), idat[:n] + bytes([idat[n] ^ (1 << (n % 8))]) + idat[n + 1:]) for n in range(len(idat))])
    assert all(0 <= status <= 12 and produced <= len(c.filtered) for status, produced, _ in got)


def test_the_tool_and_the_kernel_compile_the_same_header():
    tool = open(os.path.join(ROOT, "tools", "png_inflate_host.cpp")).read()
    kernel = open(os.path.join(ROOT, "univs_amd", "csrc", "png_inflate.hip")).read()
    assert '#include "../univs_amd/csrc/png_inflate_core.h"' in tool and '#include "png_inflate_core.h"' in kernel
    assert "png_inflate<OneLane>" in tool and "png_inflate<PngWave>" in kernel


# ---- the scorers ----------------------------------------------------------------------------------------------------------------------------
def test_reader_defaults_to_host_everywhere():
    for fn in (vps.evaluate_vps_files, vss.evaluate_vss_files, davis.evaluate_davis_files, pvos.evaluate_pvos_files, vps.VPSEvaluator.__init__,
               vss.VSSEvaluator.__init__, davis.DAVISEvaluator.__init__, pvos.PVOSEvaluator.__init__, _counts.device_stack):
        assert inspect.signature(fn).parameters["reader"].default == "host", fn
    assert _counts.device_stack(["/nowhere/at/all.png"], "host") is None         # (the host reader: the caller's own loop)
    from univs_amd import run
    base = ["--config-file", "c", "--weights", "w", "--video-dir", "d", "--output-dir", "o"]
    assert run.parse_args(base).reader == "host" and run.parse_args(base + ["--reader", "gpu"]).reader == "gpu"
    with pytest.raises(SystemExit):
        run.parse_args(base + ["--reader", "pillow"])


def test_vps_with_the_host_reader_is_the_call_without_the_argument(tmp_path):
    fx = vps_eval_cases.load("short")
    submit, truth, gt_file = vps_eval_cases.write_tree(fx, str(tmp_path))
    a = vps.evaluate_vps_files(submit, truth, gt_file, device="cpu", output_dir=str(tmp_path / "a"))
    b = vps.evaluate_vps_files(submit, truth, gt_file, device="cpu", output_dir=str(tmp_path / "b"), reader="host")
    assert a["files"] == b["files"] and repr(a["vpq"]) == repr(b["vpq"]) and repr(a["stq"]) == repr(b["stq"])
    with pytest.raises(ValueError, match="reader='pillow'"):
        vps.evaluate_vps_files(submit, truth, gt_file, device="cpu", reader="pillow")
    assert vps.VPSEvaluator({}, gt_file, truth, str(tmp_path / "e")).reader == "host"
    with pytest.raises(ValueError):
        vps.VPSEvaluator({}, gt_file, truth, str(tmp_path / "e"), reader="pillow")


def test_vss_with_the_host_reader_is_the_call_without_the_argument(tmp_path):
    fx = vss_eval_cases.load("short")
    submit, data = vss_eval_cases.write_tree(fx, str(tmp_path))
    a = vss.evaluate_vss_files(submit, data, fx["split_file"], device="cpu", output_dir=str(tmp_path / "a"))
    b = vss.evaluate_vss_files(submit, data, fx["split_file"], device="cpu", output_dir=str(tmp_path / "b"), reader="host")
    assert a["files"] == b["files"] and len(a["files"]) == 3
    with pytest.raises(ValueError, match="reader='pillow'"):
        vss.evaluate_vss_files(submit, data, fx["split_file"], device="cpu", reader="pillow")
    assert vss.VSSEvaluator({0: 1}, 255, 124, data, fx["split_file"], str(tmp_path / "e")).reader == "host"
    with pytest.raises(ValueError):
        vss.VSSEvaluator({0: 1}, 255, 124, data, fx["split_file"], str(tmp_path / "e"), reader="pillow")


def test_davis_with_the_host_reader_is_the_call_without_the_argument(tmp_path):
    fx = davis_eval_cases.load("semi_clean")
    root, res = davis_eval_cases.write_tree(fx, str(tmp_path))
    kw = dict(resolution=fx["resolution"], metrics=fx["metrics"], device="cpu")
    a = davis.evaluate_davis_files(root, res, fx["task"], output_dir=str(tmp_path / "a"), **kw)
    b = davis.evaluate_davis_files(root, res, fx["task"], output_dir=str(tmp_path / "b"), reader="host", **kw)
    assert repr(a) == repr(b)
    assert open(tmp_path / "a" / "davis-metrics.txt").read() == open(tmp_path / "b" / "davis-metrics.txt").read()
    with pytest.raises(ValueError, match="reader='pillow'"):
        davis.evaluate_davis_files(root, res, fx["task"], reader="pillow", **kw)


def test_pvos_with_the_host_reader_is_the_call_without_the_argument(tmp_path):
    fx = pvos_eval_cases.load("clean")
    data, res = pvos_eval_cases.write_tree(fx, str(tmp_path))
    a = pvos.evaluate_pvos_files(res, data, eval_decay=True, device="cpu")
    b = pvos.evaluate_pvos_files(res, data, eval_decay=True, device="cpu", reader="host")
    assert repr(a) == repr(b) and pvos.scores_text(a) == pvos.scores_text(b)
    with pytest.raises(ValueError, match="reader='pillow'"):
        pvos.evaluate_pvos_files(res, data, device="cpu", reader="pillow")
    with pytest.raises(ValueError):
        pvos.PVOSEvaluator("pvos_x", os.path.join(data, "JPEGImages"), output_dir=str(tmp_path / "e"), reader="pillow")
