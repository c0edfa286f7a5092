"""CPU: the encoder rule (univs_amd/data/jpeg_encode_rule.py) against Pillow's `save` on the corpus of tests/jpeg_encode_cases.py and
against files recorded from Pillow 12.2.0; what the corpus contains, from the rule's own coefficients; the round trip through the
decoder rule; the tables against Pillow's headers for every quality."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_encode_cases as cases
from univs_amd.data import jpeg_encode_rule as rule, jpeg_rule


@pytest.fixture(scope="module")
def coded():
    """{case name: (Blocks, Coded)}, computed once and left unchanged."""
    out = {}
    for c in cases.corpus():
        blocks = rule.scan_blocks(c.rgb, c.quality, c.sampling)
        out[c.name] = (blocks, rule.entropy_code(blocks))
    return out


def test_the_rule_gives_pillows_file_on_the_corpus(coded):
    assert len(cases.corpus()) == 12 * 3 * 3 * 5 + 3 * 4
    for c in cases.corpus():
        want = cases.pillow_file(c.rgb, c.quality, c.sampling)
        got = rule.encode_rule(c.rgb, c.quality, c.sampling)
        assert got == want, (c.name, len(got), len(want))
        assert got == rule.headers(c.rgb.shape[1], c.rgb.shape[0], c.quality, c.sampling) + coded[c.name][1].data + b"\xff\xd9"


def test_the_rule_gives_the_recorded_files(golden_dir):
    g = np.load(os.path.join(golden_dir, "g36_jpeg_encode_pil.npz"))
    assert sorted(g.files) == sorted(cases.GOLDEN_NAMES + ("recipe",))
    for c in cases.golden_cases():
        assert rule.encode_rule(c.rgb, c.quality, c.sampling) == g[c.name].tobytes(), c.name


def test_the_corpus_contains_every_hard_event(coded):
    by_name = {c.name: c for c in cases.corpus()}
    seen = dict.fromkeys(("stuffed byte", "ZRL", "no EOB", "AC category 10", "right dummy", "bottom dummy", "H = 8 mod 16 at 4:2:0"), 0)
    for name, (blocks, code) in coded.items():
        c = by_name[name]
        ac = np.abs(blocks.coef[:, 1:].astype(np.int64))
        real = blocks.dummy == 0
        # from the coefficients: a 64th coefficient that is not zero; a run of 16 zeros before a non-zero coefficient; |AC| >= 512
        no_eob = int((blocks.coef[:, 63] != 0).sum())
        nz = ac != 0
        zrl = 0
        for row in nz[nz.any(1)]:
            at = np.flatnonzero(row)
            zrl += int(((np.diff(np.concatenate([[-1], at])) - 1) >> 4).sum())      # (a ZRL per 16 zeros of a run)
        assert (no_eob, zrl) == (code.no_eob, code.zrl), name
        assert code.max_ac_category == (int(ac.max()).bit_length() if ac.size else 0)
        assert not ac[~real].any()                                   # a dummy has no AC, and the DC of the block before it
        for b in np.flatnonzero(~real):
            assert blocks.coef[b, 0] == blocks.coef[b - 1, 0] and blocks.comp[b] == blocks.comp[b - 1] == 0
        seen["stuffed byte"] += code.stuffed > 0
        seen["ZRL"] += zrl > 0
        seen["no EOB"] += no_eob > 0
        seen["AC category 10"] += code.max_ac_category == 10
        seen["right dummy"] += bool((blocks.dummy == 1).any())
        seen["bottom dummy"] += bool((blocks.dummy == 2).any())
        seen["H = 8 mod 16 at 4:2:0"] += c.sampling == "420" and c.rgb.shape[0] % 16 == 8
        assert code.max_ac_category <= 10 and code.max_dc_category <= 11
    assert all(seen.values()), seen
    # the cases named when the rule was fixed
    assert coded["noise_40x48_444_q100"][1].stuffed >= 10 and coded["noise_40x48_444_q100"][1].no_eob >= 80
    assert coded["checkerboard_40x48_444_q100"][1].max_ac_category == 10
    assert coded["morenoise_40x48_444_q30"][1].zrl >= 10 and coded["morenoise_40x48_420_q5"][1].zrl >= 1


def test_the_decoder_rule_reads_the_encoder_rule(coded):
    n = 0
    for c in cases.corpus():
        if min(c.rgb.shape[:2]) < 16 or c.quality not in (30, 100) or "smooth" in c.name:
            continue
        data = rule.encode_rule(c.rgb, c.quality, c.sampling)
        d = jpeg_rule.decode_rule(data)
        with Image.open(io.BytesIO(data)) as im:
            assert np.array_equal(d.pixels, np.asarray(im.convert("RGB"))), c.name
        # the decoder's blocks are the encoder's, natural order against zig-zag order; dummy blocks are coded like any other
        assert np.array_equal(d.blocks[:, jpeg_rule.ZIGZAG], coded[c.name][0].coef), c.name
        n += 1
    assert n >= 60


def test_tables_and_headers_are_pillows_for_every_quality():
    a = np.zeros((16, 16, 3), np.uint8)
    for quality in range(1, 101):
        p = jpeg_rule.parse_jpeg(cases.pillow_file(a, quality, "420"))
        luma, chroma = rule.quant_tables(quality)
        assert np.array_equal(p.quant[0][1], luma) and np.array_equal(p.quant[1][1], chroma)
        assert p.huff == rule.HUFF
    for sampling in cases.SAMPLINGS:
        want = cases.pillow_file(a, 90, sampling)
        head = rule.headers(16, 16, 90, sampling)
        assert want.startswith(head) and jpeg_rule.parse_jpeg(want).ecs[0] == len(head)
    with pytest.raises(ValueError, match="quality"):
        rule.quant_tables(0)
    with pytest.raises(ValueError, match="uint8"):
        rule.encode_rule(np.zeros((4, 4), np.uint8))
    with pytest.raises(KeyError):
        rule.encode_rule(a, 90, "411")


def test_the_category_guards():
    blocks = rule.scan_blocks(np.zeros((8, 8, 3), np.uint8), 90, "444")
    coef = blocks.coef.copy()
    coef[0, 5] = 1024
    with pytest.raises(jpeg_rule.JpegRuleError, match="AC category 11"):
        rule.entropy_code(blocks._replace(coef=coef))
    coef = blocks.coef.copy()
    coef[0, 0] = 2048
    with pytest.raises(jpeg_rule.JpegRuleError, match="DC category 12"):
        rule.entropy_code(blocks._replace(coef=coef))
