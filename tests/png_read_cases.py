"""The corpus of the device PNG reader, shared by tests/test_png_read_cpu.py and tests/test_png_inflate_gpu.py.  Nothing is stored: every
file is generated from seeds, because the yardstick is the installed Pillow and zlib decoding these very bytes.

  (i)   written by Pillow: blobby id maps with 2, 4, 16 and 200 palette entries (bit depths 1, 2, 4, 8), their RGB and L renderings, a
        smooth RGB gradient, RGB noise; W in {1, 7, 63, 64, 65, 130}, H in {1, 2, 63, 64, 65, 129}; level 0 (stored blocks), one image
        of more than 66 000 filtered bytes at level 0
  (ii)  hand-filtered rows through zlib.compressobj: each filter type on every row and a frame that cycles through them, bpp 1 and 3,
        levels 1 / 6 / 9 x the five strategies, some with sync / full flushes every few rows, IDAT split at arbitrary points
  (iii) streams from the deflate writer below: 15-bit codes, a code-length repeat across the literal / distance boundary, a single
        one-bit distance code, length 258 at distance 1, length 3 at distance 32768, a distance of exactly the bytes produced
  (iv)  the project's own streams (inference/png_rule.py), palette and RGB
  (v)   malformed: each records what zlib.decompress and Pillow do with it

A `Case` is a PNG file (`data`) and, for the good ones, the bytes its stream inflates to (`filtered`).
"""
import functools
import io
import struct
import zlib
from collections import namedtuple

import numpy as np

from univs_amd.inference import png_rule

# group: "pillow", "filtered", "writer", "rule" or "bad"; status: the PngStatus the inflate core must give ("bad": non-zero except for the
# filter byte, which only the unfilter launch sees); zlib_ok: zlib.decompress accepts the stream
Case = namedtuple("Case", "name group data filtered status zlib_ok")

WIDTHS = (1, 7, 63, 64, 65, 130)
HEIGHTS = (1, 2, 63, 64, 65, 129)
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE,
              "fixed": zlib.Z_FIXED}


# ---- container -----------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def png_bytes(W, H, colour_type, bit_depth, stream, palette=None, splits=(), interlace=0):
    """A PNG file around `stream`, its IDAT payload cut at `splits`."""
    out = png_rule.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bit_depth, colour_type, 0, 0, interlace))
    if palette is not None:
        out += chunk(b"PLTE", bytes(palette))
    cuts = [0, *sorted(set(s for s in splits if 0 < s < len(stream))), len(stream)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += chunk(b"IDAT", stream[a:b])
    return out + chunk(b"IEND", b"")


def pillow_png(array, palette=None, **save):
    from PIL import Image
    im = Image.fromarray(array)
    if palette is not None:
        im.putpalette(list(palette))
    buf = io.BytesIO()
    im.save(buf, format="PNG", **save)
    return buf.getvalue()


def idat_of(data):
    """(IHDR fields, concatenated IDAT payloads, payload lengths) by a plain chunk walk, independent of univs_amd.inference.png_read."""
    pos, idat, header = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", data[pos + 8:pos + 8 + n])
        if kind == b"IDAT":
            idat.append(data[pos + 8:pos + 8 + n])
        pos += 12 + n
    return header, b"".join(idat), [len(x) for x in idat]


# ---- content -------------------------------------------------------------------------------------------------------------------------
def blobs(H, W, n_ids, seed):
    """A blobby id map [H, W] uint8 with ids below n_ids."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, n_ids, (-(-H // 5), -(-W // 9)))
    return np.repeat(np.repeat(coarse, 5, axis=0), 9, axis=1)[:H, :W].astype(np.uint8)


def palette_of(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return rng.integers(0, 256, 3 * n).astype(np.uint8).tobytes()


def gradient(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(2 * x + y) % 256, (x + 3 * y) % 256, (x * y // 7 + 40) % 256], axis=-1).astype(np.uint8)


# ---- the row filters, forward ----------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_rows(raw, bpp, types):
    """The filtered bytes of the rows `raw` [H, rowbytes] uint8 with filter types[r] on row r (PNG 1.2, section 6)."""
    H, rb = raw.shape
    out = bytearray()
    for r in range(H):
        t = types[r]
        cur = [int(v) for v in raw[r]]
        up = [int(v) for v in raw[r - 1]] if r else [0] * rb
        out.append(t)
        for x in range(rb):
            a = cur[x - bpp] if x >= bpp else 0
            b = up[x]
            c = up[x - bpp] if x >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[t]
            out.append((cur[x] - pred) & 255)
    return bytes(out)


def compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, row=0):
    """zlib.compressobj on `data`; with flush_every, a sync or full flush (alternating) after every flush_every rows of `row` bytes."""
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out, step = b"", flush_every * row
    for k, i in enumerate(range(0, len(data), step)):
        out += c.compress(data[i:i + step]) + c.flush(zlib.Z_SYNC_FLUSH if k % 2 == 0 else zlib.Z_FULL_FLUSH)
    return out + c.flush()


# ---- a deflate writer: dynamic blocks from given code lengths and tokens ---------------------------------------------------------------------
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LENGTHS = [4] * 13 + [5] * 6                                      # a complete code over the 19 code-length symbols


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, n):                                         # n bits, LSB first
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):                                         # a Huffman code: MSB first
        self.put(int(format(code, f"0{n}b")[::-1], 2), n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of RFC 1951's canonical assignment."""
    code, out = 0, {}
    for n in range(1, 16):
        for s, l in enumerate(lengths):
            if l == n:
                out[s] = (code, n)
                code += 1
        code <<= 1
    return out


def dynamic_block(w, lit_lens, dist_lens, tokens, final, cl_ops=None):
    """One dynamic block into the Bits `w`.  tokens: ints (literals) and (length, distance) pairs; the end-of-block code is added.
    cl_ops: the code-length symbols (symbol, extra value) that spell lit_lens + dist_lens; default: one plain symbol per length."""
    w.put(final, 1)
    w.put(2, 2)
    w.put(len(lit_lens) - 257, 5)
    w.put(len(dist_lens) - 1, 5)
    w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(CL_LENGTHS[s], 3)
    cl = canonical(CL_LENGTHS)
    for s, extra in (cl_ops if cl_ops is not None else [(l, 0) for l in list(lit_lens) + list(dist_lens)]):
        w.code(*cl[s])
        if s >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[s])
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
            continue
        length, d = t
        i = max(k for k in range(29) if LENGTH_BASE[k] <= length) if length < 258 else 28
        w.code(*lit[257 + i])
        w.put(length - LENGTH_BASE[i], LENGTH_EXTRA[i])
        j = max(k for k in range(30) if DIST_BASE[k] <= d)
        w.code(*dist[j])
        w.put(d - DIST_BASE[j], DIST_EXTRA[j])
    w.code(*lit[256])


def stored_block(w, data, final):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put(len(data) ^ 0xFFFF, 16)
    w.out += data


def zlib_wrap(deflate, data):
    return b"\x78\x01" + deflate + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)


def play(tokens, before=b""):
    """The bytes the tokens produce after `before`."""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            for _ in range(t[0]):
                out.append(out[-t[1]])
    return bytes(out[len(before):])


def _lens(n, given):
    lens = [0] * n
    for s, l in given.items():
        lens[s] = l
    return lens


def writer_streams():
    """[(name, zlib stream, the bytes it holds)].  Every literal is in 0 .. 4, so every byte is a valid filter type and any H x (1 + W)
    factorisation of the length is a grey image."""
    out = []
    # 15-bit codes: 16 symbols with the lengths 1 .. 15, 15 (a complete code); the 15-bit ones are used
    lit = _lens(286, {0: 1, 256: 2, 1: 3, 2: 4, 257: 5, 258: 6, 259: 7, 260: 8, 261: 9, 262: 10, 263: 11, 264: 12, 285: 13, 265: 14, 3: 15, 4: 15})
    tokens = [0, 3, 4, 1, 2, 3, 3, 4, (258, 1), 4, (3, 2), (11, 2), 3, (258, 1), (5, 1), 4, 4, 3]
    w = Bits()
    dynamic_block(w, lit, [1, 1], tokens, 1)
    out.append(("codes_of_15_bits_and_258_at_1", w.bytes(), play(tokens)))
    # a repeat of the previous length (16) that starts in the literal / length lengths and ends in the distance lengths
    given = {1: 3, 2: 3, 256: 2, 284: 2, 285: 2}
    lit = _lens(286, given)
    ops, i = [], 0
    while i < 284:
        if lit[i]:
            ops.append((lit[i], 0))
            i += 1
        else:
            j = i
            while j < 284 and not lit[j]:
                j += 1
            run = j - i
            while run >= 11:
                n = min(run, 138)
                ops.append((18, n - 11))
                run -= n
            while run >= 3:
                n = min(run, 10)
                ops.append((17, n - 3))
                run -= n
            ops += [(0, 0)] * run
            i = j
    ops += [(2, 0), (16, 5 - 3)]                                    # 284: 2, then 285 and four distance lengths by one repeat
    tokens = [1, 2, 2, 1, (258, 3), 1, (227, 4), 2, (230, 2), 1]
    w = Bits()
    dynamic_block(w, lit, [2, 2, 2, 2], tokens, 1, cl_ops=ops)
    out.append(("repeat_16_across_the_boundary", w.bytes(), play(tokens)))
    # a run of zeros (18) across the boundary; the distance code is two codes of one bit at 10 and 11 (distances 33 .. 64)
    lit2 = _lens(270, {**{s: 8 for s in range(254)}, 254: 9, 255: 9, 256: 9, 257: 9})
    ops2 = [(l, 0) for l in lit2[:258]] + [(18, 12 + 10 - 11), (1, 0), (1, 0)]     # 12 zeros of 258 .. 269 and 10 distance zeros in one run
    tokens = [k % 5 for k in range(70)] + [(3, 33), (3, 40), 4, (3, 64), (3, 49), 0]
    w = Bits()
    dynamic_block(w, lit2, [0] * 10 + [1, 1], tokens, 1, cl_ops=ops2)
    out.append(("repeat_18_across_the_boundary", w.bytes(), play(tokens)))
    # a single distance code of one bit (an incomplete code that RFC 1951 allows), two blocks, a match back across the block boundary
    lit = _lens(286, {0: 2, 1: 2, 256: 3, 257: 3, 285: 2})
    t1, t2 = [0, 1, 1, 0, (258, 1), 1, (3, 1)], [(258, 1), 0, (3, 1), 1, 1]
    w = Bits()
    dynamic_block(w, lit, [1], t1, 0)
    dynamic_block(w, lit, [1], t2, 1)
    first = play(t1)
    out.append(("single_distance_code_of_one_bit", w.bytes(), first + play(t2, first)))
    # length 3 at distance 32768 and at exactly the bytes produced so far, after 32768 bytes in stored blocks
    rng = np.random.default_rng(7)
    head = rng.integers(0, 5, 32768).astype(np.uint8).tobytes()
    lit = _lens(286, {0: 2, 1: 2, 256: 3, 257: 3, 285: 2})
    dist = _lens(30, {29: 1, 0: 1})
    tokens = [(3, 32768), 1, (3, 32768), (258, 1), (3, 32768), 0, 0]              # 33038 bytes: two rows of 16519
    w = Bits()
    stored_block(w, head[:30000], 0)
    stored_block(w, b"", 0)
    stored_block(w, head[30000:], 0)
    dynamic_block(w, lit, dist, tokens, 1)
    out.append(("length_3_at_distance_32768", w.bytes(), head + play(tokens, head)))
    tokens = [3, 1, 4, 1, 0, 2, (6, 6), (3, 12), (258, 15), 2]
    lit = _lens(286, {0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 256: 3, 260: 3, 257: 4, 285: 4})
    dist = _lens(30, {4: 2, 6: 2, 7: 1})                            # codes 4 (5-6), 6 (9-12), 7 (13-16)
    w = Bits()
    dynamic_block(w, lit, dist, tokens, 1)
    out.append(("distance_of_exactly_the_bytes_produced", w.bytes(), play(tokens)))
    return [(name, zlib_wrap(s, data), data) for name, s, data in out]


def _grey_shape(n):
    """(W, H) with H (1 + W) == n, rows as long as the device takes."""
    for H in range(1, n + 1):
        if n % H == 0 and n // H - 1 <= 24576 and n // H >= 2:
            return n // H - 1, H
    raise AssertionError(n)


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------
def _pillow_cases():
    cases = []

    def add(name, array, palette=None, **save):
        data = pillow_png(array, palette, **save)
        cases.append(Case(name, "pillow", data, zlib.decompress(idat_of(data)[1]), 0, True))

    for k, n_ids in enumerate((2, 4, 16, 200)):
        pal = palette_of(n_ids, k)
        lut = np.frombuffer(pal, np.uint8).reshape(-1, 3)
        for i, W in enumerate(WIDTHS):
            H = HEIGHTS[(i + k) % 6]
            ids = blobs(H, W, n_ids, 10 * k + i)
            add(f"p{n_ids}_{W}x{H}", ids, pal)
            if n_ids in (16, 200):
                Hr = HEIGHTS[(i + k + 3) % 6]
                ids = blobs(Hr, W, n_ids, 50 + 10 * k + i)
                add(f"rgb{n_ids}_{W}x{Hr}", lut[ids])
                add(f"l{n_ids}_{W}x{Hr}", (ids.astype(np.int32) * (255 // n_ids)).astype(np.uint8))
    for W, H in ((5, 3), (13, 65), (67, 64), (131, 7)):               # sub-8-bit widths that are no multiple of 8, 4 or 2
        for n_ids in (2, 4, 16):
            add(f"p{n_ids}_{W}x{H}", blobs(H, W, n_ids, W + H + n_ids), palette_of(n_ids))
    add("gradient_130x96", gradient(96, 130))
    add("noise_65x65", np.random.default_rng(3).integers(0, 256, (65, 65, 3)).astype(np.uint8))
    add("noise_l_64x129", np.random.default_rng(4).integers(0, 256, (129, 64)).astype(np.uint8))
    add("p16_65x64_level0", blobs(64, 65, 16, 5), palette_of(16), compress_level=0)
    add("rgb_63x65_level0", gradient(65, 63), compress_level=0)
    add("l_300x230_level0", (blobs(230, 300, 200, 6).astype(np.int32) + gradient(230, 300)[..., 0] // 8).astype(np.uint8), compress_level=0)
    add("p200_130x129_level9", blobs(129, 130, 200, 8), palette_of(200), compress_level=9)
    return cases


def _filtered_cases():
    cases, rng, k = [], np.random.default_rng(11), 0
    frames = [(f"type{t}", [t] * 40) for t in range(5)] + [("cycle", [(3, 4, 0, 1, 2)[r % 5] for r in range(70)])]
    for bpp, W in ((1, 23), (3, 11)):
        for fname, types in frames:
            H = len(types)
            rb = W * bpp
            raw = (np.repeat(blobs(H, W, 9, H + bpp), bpp, axis=1).astype(np.int32) * 23 + gradient(H, rb)[..., 1] // 4 +
                   rng.integers(0, 3, (H, rb))).astype(np.uint8)
            filt = filter_rows(raw, bpp, types)
            for level in (1, 6, 9):
                for sname, strategy in STRATEGIES.items():
                    k += 1
                    stream = compress(filt, level, strategy, flush_every=(3 if k % 3 == 0 else 0), row=1 + rb)
                    cuts = {0: (), 1: (1,), 2: (len(stream) - 2, len(stream) // 2), 3: (2, 5, len(stream) - 4, len(stream) - 1)}[k % 4]
                    data = png_bytes(W, H, 2 if bpp == 3 else 0, 8, stream, splits=cuts)
                    cases.append(Case(f"{fname}_bpp{bpp}_l{level}_{sname}", "filtered", data, filt, 0, True))
    return cases


def _writer_cases():
    cases = []
    for name, stream, data in writer_streams():
        W, H = _grey_shape(len(data))
        cases.append(Case(name, "writer", png_bytes(W, H, 0, 8, stream), data, 0, True))
    return cases


def _rule_cases():
    ids = np.stack([blobs(70, 90, 11, 20), blobs(70, 90, 11, 21)])
    pal = palette_of(11)
    lut = np.frombuffer(pal, np.uint8).reshape(-1, 3)
    cases = []
    for f, s in enumerate(png_rule.deflate_maps(ids)):
        cases.append(Case(f"rule_palette_{f}", "rule", png_rule.png_file(s, 70, 90, 1, list(pal)), zlib.decompress(s), 0, True))
    for f, s in enumerate(png_rule.deflate_maps(ids, lut, 3)):
        cases.append(Case(f"rule_rgb_{f}", "rule", png_rule.png_file(s, 70, 90, 3), zlib.decompress(s), 0, True))
    return cases


def _bad_cases():
    W, H = 20, 17
    raw = (blobs(H, W, 9, 2).astype(np.int32) * 20 + gradient(H, W)[..., 0] // 3).astype(np.uint8)
    filt = filter_rows(raw, 1, [r % 5 for r in range(H)])
    good = compress(filt, 6)
    stored = compress(filt, 0)
    cases = []

    def add(name, stream, status, W=W, H=H):
        try:
            zlib.decompress(stream)
            ok = True
        except zlib.error:
            ok = False
        cases.append(Case(name, "bad", png_bytes(W, H, 0, 8, stream), None, status, ok))

    for n in (1, 2, 3, len(good) // 2, len(good) - 5, len(good) - 4, len(good) - 1):
        add(f"truncated_at_{n}", good[:n], 3)
    add("adler_flipped", good[:-2] + bytes([good[-2] ^ 0x10]) + good[-1:], 12)
    add("stored_nlen_flipped", stored[:5] + bytes([stored[5] ^ 1]) + stored[6:], 5)
    def header(cmf, flags):                                          # FCHECK makes the two bytes a multiple of 31
        return bytes([cmf, flags | (31 - ((cmf << 8) | flags) % 31) % 31])

    add("cm_is_not_8", header(0x79, 0) + good[2:], 2)
    add("window_above_32k", header(0x88, 0) + good[2:], 2)
    add("fcheck", bytes([0x78, 0x02]) + good[2:], 2)
    add("preset_dictionary", header(0x78, 0x20) + good[2:], 2)
    w = Bits()
    dynamic_block(w, _lens(286, {0: 1, 1: 1, 256: 1}), [1, 1], [0, 1], 1)
    add("over_subscribed_code", zlib_wrap(w.bytes(), bytes([0, 1])), 6, W=1, H=1)
    w = Bits()
    dynamic_block(w, _lens(286, {0: 2, 1: 2, 256: 3}), [1, 1], [0, 1], 1)
    add("incomplete_code", zlib_wrap(w.bytes(), bytes([0, 1])), 6, W=1, H=1)
    w = Bits()
    ops = [(16, 0)] + [(0, 0)] * 255 + [(1, 0)] + [(0, 0)] * 28 + [(1, 0), (1, 0)]
    dynamic_block(w, _lens(286, {256: 1}), [1, 1], [], 1, cl_ops=ops)
    add("repeat_without_a_previous_length", zlib_wrap(w.bytes(), b""), 7, W=1, H=1)
    lit = _lens(286, {0: 2, 1: 2, 256: 3, 257: 3, 285: 2})
    w = Bits()
    dynamic_block(w, lit, _lens(30, {4: 1, 0: 1}), [0, 1, 0, (3, 5), 0], 1)
    add("distance_beyond_the_output", zlib_wrap(w.bytes(), bytes(7)), 9, W=6, H=1)
    w = Bits()
    w.put(1, 1)
    w.put(3, 2)
    add("block_type_3", zlib_wrap(w.bytes(), b""), 4)
    w = Bits()
    w.put(1, 1)
    w.put(1, 2)
    for code, n in ((0x30, 8), (0xC6, 8), (0, 7)):                    # the fixed code: literal 0, symbol 286, end of block
        w.code(code, n)
    add("symbol_286", zlib_wrap(w.bytes(), bytes(1)), 8, W=1, H=1)
    w = Bits()
    w.put(1, 1)
    w.put(1, 2)
    for code, n in ((0x30, 8), (0x30, 8), (0x30, 8), (1, 7)):         # three literals, length 3 ...
        w.code(code, n)
    w.code(30, 5)                                                     # ... at distance code 30
    w.code(0, 7)
    add("distance_code_30", zlib_wrap(w.bytes(), bytes(6)), 8, W=5, H=1)
    add("more_bytes_than_the_image", good, 10, H=H - 1)
    add("fewer_bytes_than_the_image", good, 11, H=H + 1)
    five = bytearray(filt)
    five[3 * (W + 1)] = 5
    add("filter_byte_5", compress(bytes(five), 6), 0)
    return cases


@functools.lru_cache(maxsize=None)
def corpus():
    return tuple(_pillow_cases() + _filtered_cases() + _writer_cases() + _rule_cases() + _bad_cases())


def good_cases():
    return [c for c in corpus() if c.group != "bad"]


def bad_cases():
    return [c for c in corpus() if c.group == "bad"]


def host_checked_bad_cases():
    """The malformed files that may go to a GPU: those that tests/test_png_read_cpu.py runs through the host build of the decode text, plain
    and under the sanitizers, asserting `status` and the output bound of each.  That test asserts that this list is the one it covers, so
    a case added to `_bad_cases` reaches the device only together with its host check."""
    return [c for c in bad_cases() if c.status is not None and c.zlib_ok is not None]


def uncovered_files():
    """{kind: PNG bytes} of what stays with Pillow: 16-bit, grey + alpha, RGBA, 2-bit grey, 1-bit grey, interlaced."""
    a = blobs(9, 14, 4, 1)
    files = {"16-bit": pillow_png((a.astype(np.uint16) * 9000)), "LA": pillow_png(np.stack([a * 60, 255 - a], -1)),
             "RGBA": pillow_png(np.concatenate([gradient(9, 14), a[..., None] * 50], -1)),
             "1-bit grey": pillow_png(a > 1)}
    rows = np.packbits(np.repeat(a, 2, axis=1).astype(bool), axis=1)                    # any bytes will do for 2-bit grey rows
    two = filter_rows(rows[:, :4], 1, [0] * 9)
    files["2-bit grey"] = png_bytes(14, 9, 0, 2, compress(two))
    # Adam7 by hand: a 1 x 1 grey image has one pass of one row
    files["interlaced"] = png_bytes(1, 1, 0, 8, compress(bytes([0, 77])), interlace=1)
    return files


def pillow_outcome(data, rgb=False):
    """What the host reader does with the file: ("array", ndarray) or ("error", exception type)."""
    from PIL import Image
    try:
        with Image.open(io.BytesIO(data)) as im:
            return "array", np.array(im.convert("RGB") if rgb else im)
    except Exception as e:                                            # noqa: BLE001 (the type is the recorded outcome)
        return "error", type(e)
