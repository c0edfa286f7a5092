"""CPU: the rule of univs_amd/inference/png_rule.py on the frames of tests/png_cases.py.  zlib inflates every stream to the filtered
rows, Pillow opens every file to the pixels, the mode and the palette, the closed-form tokeniser equals the sequential greedy walk,
every stripe is within stripe_capacity and the all-literal stripe reaches it, and the Adler combination equals zlib.adler32."""
import io
import zlib

import numpy as np
import pytest

from tests import png_cases
from univs_amd.inference import png_rule

CASES = png_cases.cases()
NAMES = [n for n, _ in CASES]
PALETTE = [(i * 37 + j * 11) % 256 for i in range(256) for j in range(3)]


@pytest.mark.parametrize("name", NAMES)
def test_zlib_inflates_the_stream_to_the_filtered_rows(name):
    px = dict(CASES)[name]
    stream = png_rule.zlib_stream(px)
    rows = png_rule.filtered_rows(px)
    assert rows.shape == (px.shape[0], px.shape[1] * px.shape[2] + 1) and not rows[:, 0].any()
    assert zlib.decompress(stream) == rows.tobytes()
    assert stream[:2] == b"\x78\x01" and stream[-6:-4] == b"\x03\x00"
    assert int.from_bytes(stream[-4:], "big") == zlib.adler32(rows.tobytes())


@pytest.mark.parametrize("name", NAMES)
def test_pillow_opens_the_file_to_the_pixels_mode_and_palette(name):
    from PIL import Image
    px = dict(CASES)[name]
    H, W, C = px.shape
    # (a palette shorter than the ids is the caller's error on either path: Pillow then packs the pixels into fewer bits)
    for palette in ((None, PALETTE) + ((PALETTE[:30],) if px.max() < 10 else ()) if C == 1 else (None,)):
        data = png_rule.png_file(png_rule.zlib_stream(px), H, W, C, palette)
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            assert im.mode == ("RGB" if C == 3 else ("L" if palette is None else "P")) and im.size == (W, H)
            assert np.array_equal(np.asarray(im).reshape(H, W, C), px)
            # the file of the host path: the same palette comes back from both
            ref = Image.fromarray(px[..., 0] if C == 1 else px)
            if palette is not None:
                ref.putpalette(palette)
            buf = io.BytesIO()
            ref.save(buf, format="PNG")
            with Image.open(io.BytesIO(buf.getvalue())) as back:
                assert back.mode == im.mode and back.getpalette() == im.getpalette()
                assert np.array_equal(np.asarray(back), np.asarray(im))


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_tokens_equal_the_greedy_walk(name):
    px = dict(CASES)[name]
    d = px.shape[2]
    for row in np.unique(png_rule.filtered_rows(px), axis=0):
        closed, walk = png_rule.row_tokens(row, d), png_rule.row_tokens_greedy(row, d)
        assert np.array_equal(closed, walk)
        assert int(closed[:, 1].sum()) == row.shape[0] and (closed[:, 1] <= 258).all() and not (closed[:, 1] == 2).any()


def test_the_cases_hold_what_they_are_for():
    by = dict(CASES)

    def lengths(name, y=0):
        px = by[name]
        return png_rule.row_tokens(png_rule.filtered_rows(px)[y], px.shape[2])[:, 1].tolist()
    # distance 1: zeros of width 258 + r leave a remainder r after the 258-chunk; the run does not continue across the row start
    assert lengths("zeros-17x258x1") == [1, 258] and lengths("zeros-17x259x1") == [1, 258, 1]
    assert lengths("zeros-17x260x1") == [1, 258, 1, 1] and lengths("zeros-17x261x1") == [1, 258, 3]
    assert lengths("zeros-17x261x1", 5) == [1, 258, 3] and lengths("zeros-17x517x1") == [1, 258, 258, 1]
    assert lengths("zeros-1x1x1") == [1, 1] and lengths("zeros-1x2x1") == [1, 1, 1] and lengths("zeros-1x3x1") == [1, 3]
    # distance 3: the first three bytes are literals; exact remainders 0 .. 3 come from the eq patterns
    assert lengths("zeros-17x258x3") == [1, 1, 1, 258, 258, 256] and lengths("zeros-1x1x3") == [1, 1, 1, 1]
    for C in (1, 3):
        # after C + 2 + y % 3 literals: a run of 258 + y % 4, the literal that ends it, the rest of the row as one more run
        tail = [lengths("long_runs-33x517x1" if C == 1 else "long_runs-17x261x3", y) for y in range(4)]
        assert [t[C + 2 + y % 3:][:3] for y, t in enumerate(tail)] == [[258, 1, 256 if C == 1 else 258], [258, 1, 1], [258, 1, 1], [258, 3, 1]]
        assert set(lengths(f"runs_2_and_3-17x261x{C}", 0)[C:-3]) == {1, 3}
        assert max(lengths(f"period2-17x261x{C}")) == 1 and max(lengths(f"high_literals-17x261x{C}")) == 1
        assert by[f"high_literals-17x261x{C}"].min() >= 144
        assert [lengths(f"run_to_row_end-17x261x{C}", y)[-1] for y in (0, 1, 2, 9)] == [1, 1, 3, 10]
    assert png_rule.stripe_rows(24576) == 1 and png_rule.stripe_rows(6001) == 4 and png_rule.stripe_rows(3001) == 8
    assert png_rule.stripe_rows(1536) == 16 and png_rule.stripe_rows(1537) == 15 and png_rule.stripe_rows(2) == 16


@pytest.mark.parametrize("name", NAMES)
def test_every_stripe_is_within_its_capacity(name):
    px = dict(CASES)[name]
    H, W, C = px.shape
    row_len = W * C + 1
    R = png_rule.stripe_rows(row_len)
    stripes = png_rule.frame_stripes(px)
    assert len(stripes) == -(-H // R)
    for k, s in enumerate(stripes):
        rows = min(R, H - k * R)
        assert len(s) <= png_rule.stripe_capacity(rows * row_len) <= png_rule.stripe_capacity(R * row_len)
        assert s[-4:] == b"\x00\x00\xff\xff"
    assert png_rule.scratch_bytes(2, H, row_len) == 2 * len(stripes) * (16 + png_rule.stripe_capacity(R * row_len))


def test_the_all_literal_stripe_reaches_the_bound():
    for n in (1, 2, 5, 101, 24576):
        assert png_rule.stripe_capacity(n) == -(-(9 * n + 13) // 8) + 4
    # one row of 9-bit literals: 8 bits for the filter byte, 9 per pixel byte; 3 + 7 + 3 bits around them
    px = png_cases.high_literals(1, 100, 1)
    (stripe,) = png_rule.frame_stripes(px)
    assert len(stripe) == png_rule.stripe_capacity(101) == -(-(9 * 101 + 13) // 8) + 4 == 120
    (stripe,) = png_rule.frame_stripes(png_cases.high_literals(1, 24575, 1))
    assert len(stripe) == png_rule.stripe_capacity(24576)


def test_a_row_one_byte_over_the_stripe_cap_is_not_covered():
    name, px = png_cases.NOT_COVERED
    assert px.shape[1] * px.shape[2] + 1 == png_rule.STRIPE_BYTES + 1
    assert png_rule.stripe_rows(png_rule.STRIPE_BYTES + 1) is None and png_rule.stripe_rows(png_rule.STRIPE_BYTES) == 1
    assert png_rule.zlib_stream(px) is None and png_rule.deflate_maps(px[None, ..., 0]) is None


@pytest.mark.parametrize("seed", range(4))
def test_the_adler_combination_equals_zlib(seed):
    rng = np.random.default_rng(seed)
    parts = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 70000, 5)] + [b"\xff" * 24576, b""]
    ab = (1, 0)
    for p in parts:
        assert png_rule.adler_of(p) == (zlib.adler32(p) & 0xFFFF, zlib.adler32(p) >> 16)
        ab = png_rule.adler_combine(ab, png_rule.adler_of(p), len(p))
    assert (ab[1] << 16) | ab[0] == zlib.adler32(b"".join(parts))


def test_the_code_tables_are_rfc_1951s():
    # every length 3 .. 258 and both distances, decoded by zlib: a row that is one literal and one match
    for d in (1, 3):
        for L in range(3, 259):
            row = np.array([0] + [7] * (d + L), np.uint8)
            code, nbits = png_rule.token_codes([7], [L], d)
            assert 12 <= int(nbits[0]) <= 18
            px = row[1:1 + (d + L) // d * d].reshape(1, -1, d)
            assert zlib.decompress(png_rule.zlib_stream(px)) == png_rule.filtered_rows(px).tobytes()
    code, nbits = png_rule.symbol_code([0, 143, 144, 255, 256, 279, 280, 287])
    assert nbits.tolist() == [8, 8, 9, 9, 7, 7, 8, 8]
    assert code.tolist() == [0b00001100, 0b11111101, 0b000010011, 0b111111111, 0, 0b1110100, 0b00000011, 0b11100011]


def test_lut_bytes_clamp():
    lut = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    got = png_rule.lut_bytes(np.array([[-5, 0, 1, 2, 2 ** 31 - 1]], np.int32), lut, 3)
    assert got.tolist() == [[[1, 2, 3], [1, 2, 3], [4, 5, 6], [4, 5, 6], [4, 5, 6]]]
