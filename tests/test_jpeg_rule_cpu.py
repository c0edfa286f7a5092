"""CPU: the numpy statement of the JPEG decode (univs_amd/data/jpeg_rule.py) against Pillow itself on the corpus of tests/jpeg_cases.py
and against the bytes recorded from Pillow 12.2.0 (tests/golden/g35_jpeg_pil.npz, tools/gen_golden_jpeg.py); `parse_jpeg` / `covered` on the
files that are not covered and on the malformed ones; the corpus's own conditions; the public surface, whose default changes nothing."""
import inspect
import json
import os

import numpy as np
import pytest

from tests import jpeg_cases as cases
from univs_amd.data import jpeg_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_decode_rule_is_pillow_on_every_covered_file():
    for c in cases.covered_cases():
        p = rule.parse_jpeg(c.data)
        assert p.status == "ok" and rule.covered(p), (c.name, rule.why_uncovered(p))
        d = rule.decode_rule(p)
        ref = cases.pillow_pixels(c.data)
        assert d.pixels.dtype == np.uint8 and d.pixels.shape == ref.shape == (p.height, p.width, 3), c.name
        assert np.array_equal(d.pixels, ref), (c.name, int((d.pixels != ref).sum()))
        assert d.in_range, c.name
        assert d.blocks.dtype == np.int16 and d.blocks.shape == (np.prod(rule.geometry(p)[2:5]), 64), c.name


def test_decode_rule_is_the_recorded_pillow(golden_dir):
    z = np.load(os.path.join(golden_dir, "g35_jpeg_pil.npz"))
    recipe = json.loads(bytes(z["recipe"]).decode())
    assert recipe["pillow"] == "12.2.0" and len(recipe["cases"]) >= 8
    seen = set()
    for name in recipe["cases"]:
        data = bytes(z[name + "/file"])
        p = rule.parse_jpeg(data)
        assert rule.covered(p), name
        assert np.array_equal(rule.decode_rule(data).pixels, z[name + "/pixels"]), name
        seen.add((len(p.components), rule.geometry(p)[:2], p.restart_interval > 0))
    assert {s[:2] for s in seen} == {(1, (1, 1)), (3, (1, 1)), (3, (2, 1)), (3, (2, 2))} and {s[2] for s in seen} == {False, True}
    assert os.path.getsize(os.path.join(golden_dir, "g35_jpeg_pil.npz")) < 1 << 20


def test_the_corpus_meets_its_conditions():
    good = cases.covered_cases()
    assert len({c.name for c in good}) == len(good)
    seen = {"size": set(), "sampling": set(), "content": set(), "quality": set()}
    pairs = set()
    for c in good:
        p = rule.parse_jpeg(c.data)
        kind, size, sampling, q = c.name.split("_")[-4:]
        seen["size"].add((p.height, p.width)), seen["sampling"].add(sampling), seen["content"].add(kind), seen["quality"].add(int(q[1:]))
        pairs.add((sampling, kind)), pairs.add((sampling, int(q[1:])))
        expect = {"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2), "grey": (1, 1, 1)}[sampling]
        assert (len(p.components),) + rule.geometry(p)[:2] == expect, c.name
    assert seen["size"] >= set(cases.SIZES) and seen["sampling"] == set(cases.SAMPLINGS)
    assert seen["content"] >= set(cases.CONTENTS) and seen["quality"] >= set(cases.QUALITIES)
    for s in cases.SAMPLINGS:                                       # every content and every quality meets every sampling
        assert {k for (a, k) in pairs if a == s} >= set(cases.CONTENTS) | set(cases.QUALITIES), s
    standard = rule.parse_jpeg(next(c for c in good if c.name.startswith("noise_40x48_420")).data).huff
    assert all(rule.parse_jpeg(c.data).huff != standard for c in good if c.name.startswith("optimize_"))     # custom tables
    for c in good:
        p = rule.parse_jpeg(c.data)
        h, v, mx, my, per, _ = rule.geometry(p)
        if c.name.startswith("restart3_"):
            assert p.restart_interval == 3 and len(rule.unstuff(p.data, p.ecs[0])[0]) == -(-mx * my // 3) > 1, c.name
        elif c.name.startswith("restartrow_"):
            assert p.restart_interval == mx and len(rule.unstuff(p.data, p.ecs[0])[0]) == my > 1, c.name
        else:
            assert p.restart_interval == 0
    # the chunk-crossing file: one interval, more than 1024 subsequences of 32 and of 64 bits
    p = rule.parse_jpeg(cases.chunk_crossing().data)
    (one,), status = rule.unstuff(p.data, p.ecs[0])
    assert status == "ok" and len(one) >= 8192 and 8 * len(one) > 1024 * 64
    # the clamp of the colour conversion is pushed: a patches file whose unclamped values leave [0, 255]
    p = rule.parse_jpeg(next(c for c in good if c.name.startswith("patches_") and "_444_" in c.name).data)
    planes, _ = rule.planes_from_blocks(p, rule.decode_blocks(p))
    y, cb, cr = (a[:p.height, :p.width].astype(np.int64) for a in planes)
    r = y + ((91881 * (cr - 128) + 32768) >> 16)
    assert r.max() > 255 or r.min() < 0


def test_files_that_are_not_covered_say_why():
    got = {}
    for kind, data in cases.uncovered_files().items():
        p = rule.parse_jpeg(data)
        assert p.status == "ok" and not rule.covered(p), kind
        got[kind] = rule.why_uncovered(p)
        with pytest.raises(ValueError, match="not covered"):
            rule.decode_rule(data)
        assert cases.host_read(data)[0] == "pixels"                  # the host reader takes them
    assert got == cases.UNCOVERED_REASONS
    good = rule.parse_jpeg(cases.covered_cases()[0].data)
    assert rule.covered(good._replace(orientation=1)) and not rule.covered(good._replace(orientation=3))
    assert not rule.covered(good._replace(precision=12)) and not rule.covered(good._replace(sof=9)) and not rule.covered(good._replace(colour="rgb"))
    assert not rule.covered(good._replace(width=15)) and not rule.covered(good._replace(height=16385))
    tq = good.components[0][3]
    assert not rule.covered(good._replace(quant={**good.quant, tq: (1, good.quant[tq][1])}))     # a 16-bit quantisation table
    assert not rule.covered(good._replace(scan=good.scan[:1] + good.scan[-1:]))                  # a scan that does not hold all components
    c444 = rule.parse_jpeg(next(c for c in cases.covered_cases() if "_444_" in c.name).data)
    tall = ((c444.components[0][0], 1, 2, c444.components[0][3]),) + c444.components[1:]
    assert rule.why_uncovered(c444._replace(components=tall)) == "sampling 1x2 1x1 1x1"          # 4:4:0 stays with Pillow


def test_parse_statuses_of_files_that_do_not_parse():
    good = cases.covered_cases()[0].data
    assert rule.parse_jpeg(b"").status == rule.parse_jpeg(b"\x89PNG\r\n\x1a\n" + bytes(20)).status == "not a JPEG file"
    assert rule.parse_jpeg(good[:30]).status == "truncated in the headers"
    assert rule.parse_jpeg(good[:2] + b"\x00\x00" + good[2:]).status == "bytes that are no marker between the segments"
    assert rule.parse_jpeg(good[:2] + b"\xff\xd9" + good[2:]).status == "end of image before a scan"
    sof = next(s for s in cases.segments(good) if s[0] == 0xC0)
    assert rule.parse_jpeg(good[:sof[1]] + good[sof[2]:]).status == "no frame header before the scan"
    assert rule.parse_jpeg(good[:sof[2]] + good[sof[1]:]).status == "two frame headers"
    for data in (b"", good[:30]):
        assert not rule.covered(rule.parse_jpeg(data))


def test_malformed_files_never_come_out_as_wrong_pixels():
    bad = cases.malformed_files()
    assert {"truncated in the headers", "truncated in the middle", "flipped bit", "huffman count overflow", "more blocks than data", "dri doubled",
            "dri removed"} <= set(bad) and sum(k.startswith("truncated") for k in bad) >= 4
    outcomes = {}
    for name, data in bad.items():
        p = rule.parse_jpeg(data)
        try:
            d = rule.decode_rule(p) if rule.covered(p) else None
        except rule.JpegRuleError as e:
            outcomes[name] = "rule: " + str(e).split(",")[0]
            continue
        if d is None:
            outcomes[name] = "parse: " + rule.why_uncovered(p)
            continue
        kind, ref = cases.host_read(data)                            # status OK: then the pixels are Pillow's
        assert kind == "pixels" and np.array_equal(d.pixels, ref), name
        outcomes[name] = "pixels"
    assert outcomes["huffman count overflow"] == "parse: bad DHT" and outcomes["truncated in the headers"] == "parse: truncated in the headers"
    assert outcomes["more blocks than data"] == "rule: data exhausted before the expected number of blocks"
    assert outcomes["dri doubled"].startswith("rule: 3 restart intervals") and outcomes["dri removed"].startswith("rule: 3 restart intervals")
    assert all(v == "rule: no end-of-image marker after the data" for k, v in outcomes.items() if k.startswith("truncated") and "headers" not in k)


def test_the_range_conditions_are_reported():
    data = cases.oversized_product()
    p = rule.parse_jpeg(data)
    assert rule.covered(p)
    d = rule.decode_rule(p)
    assert int(d.blocks[0, 0]) == 1020 and int(p.quant[p.components[0][3]][1][0]) == 255 and not d.in_range
    px, ok = rule.idct_islow(np.array([[1, 0] + [0] * 62], np.int16), np.full(64, 255, np.uint16))
    assert ok and px.shape == (1, 8, 8)
    assert not rule.idct_islow(np.array([[130] + [0] * 63], np.int16), np.full(64, 255, np.uint16))[1]      # 33150 > 32767
    assert not rule.idct_islow(np.array([[128] + [0] * 63], np.int16), np.full(64, 255, np.uint16))[1]      # 32640 / 8 = 4080 > 511


def test_decode_defaults_to_host_everywhere():
    from univs_amd import data, run
    from univs_amd.data import images, mapper, vos_mapper
    assert inspect.signature(images.read_images).parameters["decode"].default == "host"
    assert inspect.signature(mapper.VideoTestMapper.__init__).parameters["decode"].default == "host"
    assert inspect.signature(mapper.VideoTestMapper.from_config).parameters["decode"].default == "host"
    assert data.read_images is images.read_images
    m = vos_mapper.VOSTestMapper(360, 640)
    assert (m.decode, m.resize) == ("host", "host")
    with pytest.raises(ValueError, match="needs resize=\"gpu\""):
        mapper.VideoTestMapper(360, 640, decode="gpu", resize="host")
    with pytest.raises(ValueError, match="decode='pillow'"):
        mapper.VideoTestMapper(360, 640, decode="pillow")
    with pytest.raises(ValueError, match="decode='pillow'"):
        images.read_images([], decode="pillow")
    base = ["--config-file", "c", "--weights", "w", "--video-dir", "d", "--output-dir", "o"]
    assert run.parse_args(base).decode == "host" and run.parse_args(base + ["--decode", "gpu"]).decode == "gpu"
    with pytest.raises(SystemExit):
        run.parse_args(base + ["--decode", "pillow"])


def test_read_images_on_the_host_is_read_image(tmp_path):
    from univs_amd.data import images
    paths = []
    for i, c in enumerate(cases.covered_cases()[:3]):
        paths.append(str(tmp_path / f"{i}.jpg"))
        open(paths[-1], "wb").write(c.data)
    for fmt in ("RGB", "BGR"):
        got = images.read_images(paths, format=fmt)
        assert all(isinstance(a, np.ndarray) and np.array_equal(a, images.read_image(p, fmt)) for a, p in zip(got, paths))
