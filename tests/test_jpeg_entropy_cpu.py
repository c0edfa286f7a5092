"""CPU: the entropy decoder of the device JPEG reader (csrc/jpeg_entropy_core.h) compiled for the host by tools/jpeg_entropy_host.cpp, a
stand-alone program that is never loaded into Python, plain and with the address and undefined-behaviour sanitizers.  Every corpus file
is decoded serially and by the kernel's subsequence schedule (emulated lane by lane) at 32, 64 and 1024 bits per subsequence: the
coefficient blocks equal `decode_rule`'s, every lane's exit state is the serial decode's, and the rounds stay within their bound.  The
malformed files, every prefix of one small stream and a one-bit corruption at each of its bytes end with a status and inside the file's
regions (each interval and the block buffer are heap blocks of exactly their sizes)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_cases as cases
from univs_amd.data import jpeg_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG = 1024                                                            # csrc/jpeg_entropy_core.h: JPEG_WG
SUBSEQ = (32, 64, 1024)
EOI, EXHAUSTED, RESTART = 512, 16, 32                                # csrc/jpeg_entropy_core.h: JpegStatus


def _compiler():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return [shutil.which(c)]
    from univs_amd import build
    return [build._hipcc(), "-x", "c++"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("jpeg_entropy_host") / request.param)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else []
    cc = _compiler()
    if flags and "clang" not in subprocess.run([cc[0], "--version"], capture_output=True, text=True).stdout:
        flags += ["-static-libasan", "-static-libubsan"]            # (clang's default; the program then needs nothing from its environment)
    if "hipcc" in cc[0] and flags:
        flags = [a for f in flags for a in ("-Xarch_host", f)]
    subprocess.run([*cc, "-O1", "-g", "-std=c++17", *flags, os.path.join(ROOT, "tools", "jpeg_entropy_host.cpp"), "-o", out], check=True)
    return out


def _fnv(data):
    h = 1469598103934665603
    for x in data:
        h = ((h ^ x) * 1099511628211) & (2 ** 64 - 1)
    return h


def _record(p, subseq_bits, raw=None):
    h, v, mx, my, per, _ = rule.geometry(p)
    tables = rule.table_bytes(p)
    raw = p.data[p.ecs[0]:] if raw is None else raw
    return struct.pack("<6i", per, h * v, p.restart_interval, mx * my, subseq_bits, len(tables)) + tables.tobytes() + struct.pack("<Q", len(raw)) + raw


def _run(program, records):
    """[(serial status, schedule status, blocks, serial digest, schedule digest, rounds, lanes, states equal)] through one plain subprocess of
    the program, in the environment as it is: the sanitizers' runtimes are linked into the program."""
    r = subprocess.run([program], input=b"".join(records), capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(records)
    return [(int(a), int(b), int(c), int(d, 16), int(e, 16), int(f), int(g), int(h)) for a, b, c, d, e, f, g, h in (line.split() for line in lines)]


def test_serial_and_scheduled_decode_give_the_rules_blocks(host_program):
    good = cases.covered_cases()
    parsed = [rule.parse_jpeg(c.data) for c in good]
    digests = [_fnv(rule.decode_blocks(p).astype("<i2").tobytes()) for p in parsed]
    got = _run(host_program, [_record(p, sb) for p in parsed for sb in SUBSEQ])
    crossed = set()
    for i, (c, p) in enumerate(zip(good, parsed)):
        for j, sb in enumerate(SUBSEQ):
            serial, sched, nblocks, d_serial, d_sched, rounds, lanes, states = got[3 * i + j]
            assert (serial, sched) == (0, 0), (c.name, sb, serial, sched)
            assert nblocks == np.prod(rule.geometry(p)[2:5]) and d_serial == d_sched == digests[i], (c.name, sb)
            assert states == 1, (c.name, sb)                         # the fixpoint is the serial decode's states
            assert 1 <= lanes <= WG and rounds <= max(lanes - 1, 0), (c.name, sb, rounds, lanes)
            intervals = rule.unstuff(p.data, p.ecs[0])[0]
            if max(len(x) for x in intervals) * 8 > WG * sb:
                crossed.add(sb)
                assert lanes == WG
    assert crossed >= {32, 64}                                       # the chunk-crossing file crosses at both small sizes


def test_malformed_files_end_with_a_status_or_with_pillows_pixels(host_program):
    bad = {k: v for k, v in cases.malformed_files().items() if rule.covered(rule.parse_jpeg(v))}
    assert len(bad) >= 8
    names = sorted(bad)
    got = _run(host_program, [_record(rule.parse_jpeg(bad[k]), sb) for k in names for sb in SUBSEQ])
    for i, k in enumerate(names):
        p = rule.parse_jpeg(bad[k])
        for j, sb in enumerate(SUBSEQ):
            serial, sched, _, d_serial, d_sched, _, _, _ = got[3 * i + j]
            assert (serial == 0) == (sched == 0), (k, sb, serial, sched)
            if serial == 0:                                          # then the blocks are the rule's, whose pixels are Pillow's (test_jpeg_rule_cpu)
                assert d_serial == d_sched == _fnv(rule.decode_blocks(p).astype("<i2").tobytes()), (k, sb)
        serial = got[3 * i][0]
        if k.startswith("truncated"):
            assert serial & EOI, (k, serial)
        if k == "more blocks than data":
            assert serial & EXHAUSTED, serial
        if k.startswith("dri"):
            assert serial & RESTART, serial
        if k == "flipped bit":
            assert serial == 0                                       # (this flip changes a magnitude only: Pillow's pixels, asserted in test_jpeg_rule_cpu)


def test_prefixes_and_bit_flips_of_a_small_stream_end_inside_their_regions(host_program):
    c = next(c for c in cases.covered_cases() if c.name.startswith("restart3_optimize_17x31_420"))
    p = rule.parse_jpeg(c.data)
    raw = p.data[p.ecs[0]:]
    assert 100 < len(raw) < 4000
    prefixes = _run(host_program, [_record(p, 32, raw[:n]) for n in range(len(raw))])
    assert all(serial != 0 and sched != 0 for serial, sched, *_ in prefixes)     # no prefix has its EOI
    flips = _run(host_program, [_record(p, 32, raw[:n] + bytes([raw[n] ^ (1 << (n % 8))]) + raw[n + 1:]) for n in range(len(raw))])
    assert all(0 <= serial < 1024 and 0 <= sched < 1024 and (serial == 0) == (sched == 0) for serial, sched, *_ in flips)
    same = [a[3] == a[4] for a in flips if a[0] == 0]
    assert len(same) > 0 and all(same)                               # where both decode, they decode the same blocks
    flips64 = _run(host_program, [_record(p, 64, raw[:n] + bytes([raw[n] ^ (1 << (n % 8))]) + raw[n + 1:]) for n in range(0, len(raw), 3)])
    assert all((serial == 0) == (sched == 0) for serial, sched, *_ in flips64)


def test_the_tool_and_the_kernel_compile_the_same_header():
    tool = open(os.path.join(ROOT, "tools", "jpeg_entropy_host.cpp")).read()
    kernel = open(os.path.join(ROOT, "univs_amd", "csrc", "jpeg_decode.hip")).read()
    assert '#include "../univs_amd/csrc/jpeg_entropy_core.h"' in tool and '#include "jpeg_entropy_core.h"' in kernel
    for text in (tool, kernel):
        assert "jpeg_decode_span<false>" in text and "jpeg_decode_span<true>" in text and "jpeg_byte_role(" in text and "jpeg_build_table(" in text
    core = open(os.path.join(ROOT, "univs_amd", "csrc", "jpeg_entropy_core.h")).read()
    assert "constexpr int JPEG_WG = %d;" % WG in core
