"""The PNG files of the result writers when the device encodes them, stated in numpy: the yardstick of csrc/png_deflate.hip and the
document of the format.  Integer arithmetic only.  Pinned to the DECODERS of zlib and Pillow (every stream inflates to the filtered
rows, every file opens to the pixels, mode and palette), not to any encoder: the bytes differ from `PIL.Image.save`'s.

A frame is H rows of W pixels of C in {1, 3} bytes.  Its filtered row is one byte 0 (PNG filter "None") and the W C pixel bytes:
row_len = W C + 1; the match distance is d = C (the same channel of the pixel before).

Tokens of a row (matches never cross a row start):   eq[i] = i >= d and row[i] == row[i - d];  a position with eq false is a literal;
a maximal run [s, s + n) of eq-true positions is cut greedily into chunks of 258: a chunk of L >= 3 is one match (L, d) at its first
position, a last chunk of 1 or 2 is that many literals.  `row_tokens` is this closed form, `row_tokens_greedy` the sequential walk
"the longest distance-d match at the cursor, at most 258, taken when >= 3" it equals (tests/test_png_rule_cpu.py compares them).

Codes: RFC 1951's fixed Huffman code (BTYPE = 01).  Literal / length symbols 0-143: 8 bits 0x30 + v; 144-255: 9 bits 0x190 + v - 144;
256-279: 7 bits v - 256; 280-287: 8 bits 0xC0 + v - 280.  Huffman codes enter the LSB-first bit stream bit-reversed, extra bits as they
are.  Lengths follow the RFC's table (`LENGTH_BASE` / `LENGTH_EXTRA`; 258 is symbol 285 without extra bits); the distance code is 5
bits, reversed: distances 1 and 3 are codes 0 and 2 without extra bits.

Stripes: R = stripe_rows(row_len) consecutive rows are one deflate block -- 3 header bits (BFINAL 0, BTYPE 01), the rows' tokens, the
end-of-block symbol (7 zero bits), then an empty stored block (3 zero bits, padding to a byte, 00 00 FF FF) -- so a stripe is a whole
number of bytes and stripes concatenate.  R is part of the format: the largest R <= STRIPE_ROWS_MAX with R row_len <= STRIPE_BYTES
(what the kernel keeps in LDS); a row longer than STRIPE_BYTES is not covered (None).  A stripe of n filtered bytes takes at most
stripe_capacity(n) = ceil((9 n + 13) / 8) + 4 bytes: a literal costs at most 9 bits, a match at most 18 for at least 3 bytes.

The zlib stream of a frame: 78 01, the stripes, 03 00 (a final fixed block that holds only end-of-block), the big-endian Adler-32 of
all filtered rows.  The file: signature, IHDR (8 bits deep; colour type 3 with a palette, 0 without, 2 for C = 3), PLTE when a palette
is given (the entries `putpalette` would store, at most 256), one IDAT, IEND; chunk CRCs from zlib.crc32.
"""
import struct
import zlib

import numpy as np

STRIPE_ROWS_MAX = 16
STRIPE_BYTES = 24 * 1024
MAX_MATCH = 258
ADLER = 65521
SIGNATURE = b"\x89PNG\r\n\x1a\n"

# RFC 1951, 3.2.5: length symbols 257 .. 285, their base lengths and extra bits
LENGTH_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
LENGTH_EXTRA = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0])
DISTANCE_CODE = {1: 0, 3: 2}


def stripe_rows(row_len):
    """R, or None where a row does not fit a stripe."""
    if row_len > STRIPE_BYTES:
        return None
    return max(1, min(STRIPE_ROWS_MAX, STRIPE_BYTES // row_len))


def stripe_capacity(n):
    return (9 * n + 13 + 7) // 8 + 4


def scratch_bytes(N, H, row_len):
    """What the kernel's `scratch` holds for N frames: four int32 per stripe and a slot of stripe_capacity(R row_len) bytes per stripe."""
    R = stripe_rows(row_len)
    S = -(-H // R)
    return N * S * (16 + stripe_capacity(R * row_len))


def lut_bytes(src, lut=None, channels=1):
    """The pixel bytes [.., H, W, C] of an id map: lut[clamp(id, 0, K - 1)], identity without a table."""
    src = np.asarray(src)
    if lut is None:
        assert src.dtype == np.uint8 and channels == 1
        return src[..., None]
    lut = np.asarray(lut, dtype=np.uint8).reshape(-1, channels)
    return lut[np.clip(src.astype(np.int64), 0, lut.shape[0] - 1)]


def filtered_rows(pixels):
    """uint8 [H, W, C] -> uint8 [H, W C + 1]."""
    H = pixels.shape[0]
    return np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(pixels, dtype=np.uint8).reshape(H, -1)], axis=1)


# ------------------------------------------------------------------------------------------------------------------
# tokens: (position, length) with length 1 = the literal row[position], length >= 3 = a match of that length at distance d
# ------------------------------------------------------------------------------------------------------------------
def row_tokens(row, d):
    """The closed form: int64 [n_tokens, 2]."""
    n = row.shape[0]
    i = np.arange(n)
    eq = np.zeros(n, bool)
    eq[d:] = row[d:] == row[:-d]
    false_at = np.where(~eq, i, -1)
    start = np.maximum.accumulate(false_at) + 1                         # the run's first position (eq[0] is false)
    nxt = np.where(~eq, i, n)
    end = np.minimum.accumulate(nxt[::-1])[::-1]                        # one past the run's last position
    k = i - start
    chunk_len = np.minimum(MAX_MATCH, (end - start) - (k // MAX_MATCH) * MAX_MATCH)
    literal = ~eq | (chunk_len < 3)
    match = eq & (chunk_len >= 3) & (k % MAX_MATCH == 0)
    keep = literal | match
    return np.stack([i[keep], np.where(match, chunk_len, 1)[keep]], axis=1).astype(np.int64)


def row_tokens_greedy(row, d):
    """The sequential walk: the longest distance-d match at the cursor, at most 258, taken when >= 3."""
    n, i, out = row.shape[0], 0, []
    while i < n:
        L = 0
        while i >= d and i + L < n and L < MAX_MATCH and row[i + L] == row[i + L - d]:
            L += 1
        if L >= 3:
            out.append((i, L))
            i += L
        else:
            out.append((i, 1))
            i += 1
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------------
# codes
# ------------------------------------------------------------------------------------------------------------------
def _reverse(code, nbits):
    out = np.zeros_like(code)
    for b in range(9):
        out |= ((code >> b) & 1) << (nbits - 1 - b).clip(0)
    return out


def symbol_code(sym):
    """(bits as they enter the LSB-first stream, their number) of literal / length symbols."""
    sym = np.asarray(sym, dtype=np.int64)
    code = np.select([sym < 144, sym < 256, sym < 280], [0x30 + sym, 0x190 + sym - 144, sym - 256], 0xC0 + sym - 280)
    nbits = np.select([sym < 144, sym < 256, sym < 280], [8, 9, 7], 8)
    return _reverse(code, nbits), nbits


def token_codes(values, lengths, d):
    """(code, nbits) per token: a literal's symbol, or a match's length symbol, extra bits and distance code in one word (<= 18 bits)."""
    values, lengths = np.asarray(values, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    is_match = lengths >= 3
    idx = np.searchsorted(LENGTH_BASE, np.where(is_match, lengths, 3), side="right") - 1
    code, nbits = symbol_code(np.where(is_match, 257 + idx, values))
    extra, ebits = np.where(is_match, lengths - LENGTH_BASE[idx], 0), np.where(is_match, LENGTH_EXTRA[idx], 0)
    dist = int(_reverse(np.array([DISTANCE_CODE[d]]), np.array([5]))[0])
    code = code | (extra << nbits) | np.where(is_match, dist << (nbits + ebits), 0)
    return code, nbits + ebits + np.where(is_match, 5, 0)


def stripe_bytes(rows, d):
    """One stripe's deflate blocks as bytes: rows uint8 [r, row_len]."""
    values, lengths = [], []
    for row in rows:
        t = row_tokens(row, d)
        values.append(row[t[:, 0]])
        lengths.append(t[:, 1])
    code, nbits = token_codes(np.concatenate(values), np.concatenate(lengths), d)
    at = 3 + np.concatenate([[0], np.cumsum(nbits)])                    # the 3 header bits: BFINAL 0, BTYPE 01 = the bits 0, 1, 0
    total = int(at[-1]) + 7 + 3                                         # end of block, the stored block's header
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    bits[1] = 1
    b = np.arange(18)[None, :]
    on = (b < nbits[:, None]) & (((code[:, None] >> b) & 1) == 1)
    bits[(at[:-1, None] + b)[on]] = 1
    return np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"


def adler_of(data):
    """(a, b) of Adler-32 over `data` from the start value 1."""
    x = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = x.shape[0]
    return int((1 + x.sum()) % ADLER), int((n + ((n - np.arange(n)) * x).sum()) % ADLER)


def adler_combine(ab1, ab2, len2):
    (a1, b1), (a2, b2) = ab1, ab2
    return (a1 + a2 - 1) % ADLER, (b1 + b2 + len2 * (a1 - 1)) % ADLER


def frame_stripes(pixels):
    """The stripes of one frame (uint8 [H, W, C]) as a list of bytes, or None where a row is beyond the stripe cap."""
    rows = filtered_rows(pixels)
    R = stripe_rows(rows.shape[1])
    if R is None:
        return None
    d = pixels.shape[2]
    return [stripe_bytes(rows[y:y + R], d) for y in range(0, rows.shape[0], R)]


def zlib_stream(pixels):
    """The zlib stream of one frame, or None where it is not covered."""
    stripes = frame_stripes(pixels)
    if stripes is None:
        return None
    rows = filtered_rows(pixels)
    R = stripe_rows(rows.shape[1])
    ab = (1, 0)
    for y in range(0, rows.shape[0], R):
        part = rows[y:y + R].tobytes()
        ab = adler_combine(ab, adler_of(part), len(part))
    return b"\x78\x01" + b"".join(stripes) + b"\x03\x00" + struct.pack(">I", (ab[1] << 16) | ab[0])


def deflate_maps(src, lut=None, channels=1):
    """What png_ops.deflate_maps returns, on the host: one zlib stream per frame of the id maps [N, H, W], or None."""
    px = lut_bytes(src, lut, channels)
    if stripe_rows(px.shape[2] * channels + 1) is None:
        return None
    return [zlib_stream(p) for p in px]


# ------------------------------------------------------------------------------------------------------------------
# the container
# ------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def palette_bytes(palette):
    """The PLTE data `PIL.Image.putpalette(palette)` + `save` stores: the given RGB triples, at most 256 and at least one of them (zeros
    where the list ends inside a triple or is empty)."""
    p = bytes(bytearray(palette))
    n = max(min(len(p) // 3, 256), 1)
    return p[:3 * n] + b"\x00" * (3 * n - len(p[:3 * n]))


def png_file(stream, H, W, channels=1, palette=None):
    """The file around one frame's zlib stream."""
    colour = 2 if channels == 3 else (3 if palette is not None else 0)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, colour, 0, 0, 0))
    if colour == 3:
        out += chunk(b"PLTE", palette_bytes(palette))
    return out + chunk(b"IDAT", stream) + chunk(b"IEND", b"")
