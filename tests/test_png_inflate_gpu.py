"""GPU: csrc/png_inflate.hip on the corpus of tests/png_read_cases.py.  The inflated bytes equal `zlib.decompress`'s and the planes equal
`np.array(PIL.Image.open(...))` (rgb: of `.convert("RGB")`) bit for bit, with uncovered="raise", so that no covered file can pass through
Pillow; guard bands around and between the files' regions stay untouched; malformed files fall back and do what the host reader does
while the good files of the same call stay right; uncovered kinds fall back; id maps written by png="gpu" come back."""
import functools

import numpy as np
import pytest
import torch

from tests import png_read_cases as cases
from univs_amd import png_ops, png_read_ops
from univs_amd.inference import png_read, png_rule

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARKER = 0xA5
GROUPS = ("pillow", "filtered", "writer", "rule")


@functools.lru_cache(maxsize=None)
def _pillow(name, rgb):
    case = {c.name: c for c in cases.corpus()}[name]
    kind, value = cases.pillow_outcome(case.data, rgb)
    assert kind == "array"
    return value


def _markers_intact(res, margin, gap):
    for buf, offs, sizes in ((res.filtered, res.filt_offsets, res.filt_sizes), (res.out, res.out_offsets, res.out_sizes)):
        host = buf.cpu().numpy()
        keep = np.ones(len(host), bool)
        for o, n in zip(offs[:-1], sizes):
            keep[int(o):int(o) + int(n)] = False
        assert keep.sum() == 2 * margin + gap * len(sizes)
        assert (host[keep] == MARKER).all()


@pytest.mark.parametrize("group", GROUPS)
def test_inflated_bytes_equal_zlib_and_statuses_are_zero(group):
    cs = [c for c in cases.good_cases() if c.group == group]
    res = png_read_ops.read_covered([png_read.parse_png(c.data) for c in cs], DEV, margin=256, gap=64, marker=MARKER)
    assert res.status.tolist() == [0] * len(cs)
    filt = res.filtered.cpu().numpy()
    for c, o, n in zip(cs, res.filt_offsets, res.filt_sizes):
        assert n == len(c.filtered) and filt[int(o):int(o) + int(n)].tobytes() == c.filtered, c.name
    _markers_intact(res, 256, 64)


@pytest.mark.parametrize("rgb", [False, True])
@pytest.mark.parametrize("group", GROUPS)
def test_planes_equal_pillow_and_nothing_falls_back(group, rgb):
    cs = [c for c in cases.good_cases() if c.group == group]
    planes = png_read_ops.read_pngs_device([c.data for c in cs], DEV, rgb=rgb, uncovered="raise")
    assert len(planes) == len(cs)
    for c, p in zip(cs, planes):
        want = _pillow(c.name, rgb)
        assert p.dtype == torch.uint8 and p.is_cuda and tuple(p.shape) == want.shape, c.name
        assert torch.equal(p.cpu(), torch.from_numpy(want)), c.name


def test_forty_mixed_files_in_one_call_with_guard_bands():
    good = cases.good_cases()
    by_group = [[c for c in good if c.group == g] for g in GROUPS]
    cs = [by_group[i % 4][(i * 7) % len(by_group[i % 4])] for i in range(40)]      # every group, sizes, kinds and bit depths interleaved
    assert len({c.group for c in cs}) >= 3 and len({png_read.parse_png(c.data).bit_depth for c in cs}) >= 3
    for rgb in (False, True):
        res = png_read_ops.read_covered([png_read.parse_png(c.data) for c in cs], DEV, rgb=rgb, margin=256, gap=100, marker=MARKER)
        assert res.status.tolist() == [0] * 40
        for c, p in zip(cs, res.planes):
            assert torch.equal(p.cpu(), torch.from_numpy(_pillow(c.name, rgb))), c.name
        _markers_intact(res, 256, 100)


def test_malformed_files_beside_good_ones():
    """Only `cases.host_checked_bad_cases()` go to the device: the streams tests/test_png_read_cpu.py runs through the host build of the
    same decode text under the address and undefined-behaviour sanitizers; their statuses there are the ones expected here."""
    bad, good = cases.host_checked_bad_cases(), cases.good_cases()[::29]
    order = []
    for i, b in enumerate(bad):
        order += [b, good[i % len(good)]]
    res = png_read_ops.read_covered([png_read.parse_png(c.data) for c in order], DEV, margin=256, gap=64, marker=MARKER)
    for c, st, p in zip(order, res.status.tolist(), res.planes):
        if c.group != "bad":
            assert st == 0 and torch.equal(p.cpu(), torch.from_numpy(_pillow(c.name, False))), c.name
        else:
            assert st == (13 if c.name == "filter_byte_5" else c.status), c.name
    _markers_intact(res, 256, 64)


@pytest.mark.parametrize("name", [c.name for c in cases.host_checked_bad_cases()])
def test_a_malformed_file_falls_back_and_does_what_the_host_reader_does(name):
    c = {c.name: c for c in cases.host_checked_bad_cases()}[name]
    good = cases.good_cases()[0]
    kind, value = cases.pillow_outcome(c.data)
    with pytest.raises(png_read_ops.UncoveredPng, match="file 1 has status"):
        png_read_ops.read_pngs_device([good.data, c.data], DEV, uncovered="raise")
    if kind == "error":
        with pytest.raises(value):
            png_read_ops.read_pngs_device([good.data, c.data], DEV)
    else:
        planes = png_read_ops.read_pngs_device([good.data, c.data], DEV)
        assert torch.equal(planes[1].cpu(), torch.from_numpy(value))
        assert torch.equal(planes[0].cpu(), torch.from_numpy(_pillow(good.name, False)))


def test_uncovered_kinds_fall_back_and_raise_names_the_file():
    good = cases.good_cases()[0]
    for kind, data in cases.uncovered_files().items():
        want = cases.pillow_outcome(data)[1]
        planes = png_read_ops.read_pngs_device([good.data, data], DEV)
        got = planes[1].cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), kind
        with pytest.raises(png_read_ops.UncoveredPng, match="file 1 is not covered"):
            png_read_ops.read_pngs_device([good.data, data], DEV, uncovered="raise")
    with pytest.raises(png_read_ops.UncoveredPng, match="file 0 does not parse"):
        png_read_ops.read_pngs_device([b"no png at all"], DEV, uncovered="raise")
    assert png_read_ops.read_pngs_device([], DEV) == []


def test_id_maps_written_by_the_device_come_back():
    ids = np.stack([cases.blobs(70, 90, 11, s) for s in (1, 2, 3)])
    pal = cases.palette_of(11)
    lut = np.frombuffer(pal, np.uint8).reshape(-1, 3)
    src = torch.from_numpy(ids).to(DEV)
    files = png_ops.png_files(png_ops.deflate_maps(src), 70, 90, 1, list(pal))
    back = png_read_ops.read_pngs_device(files, DEV, uncovered="raise")
    assert torch.equal(torch.stack(back), src)
    rgb = png_read_ops.read_pngs_device(files, DEV, rgb=True, uncovered="raise")
    assert torch.equal(torch.stack(rgb).cpu(), torch.from_numpy(lut[ids]))
    files = png_ops.png_files(png_ops.deflate_maps(src, torch.from_numpy(lut.copy()).to(DEV), 3), 70, 90, 3)
    assert files == [png_rule.png_file(s, 70, 90, 3) for s in png_rule.deflate_maps(ids, lut, 3)]
    back = png_read_ops.read_pngs_device(files, DEV, uncovered="raise")
    assert torch.equal(torch.stack(back).cpu(), torch.from_numpy(lut[ids]))
