"""Baseline JPEG as Pillow encodes it, stated once in numpy: the yardstick of csrc/jpeg_encode.hip, the counterpart of data/jpeg_rule.py.
No GPU.

Pillow links libjpeg-turbo and `Image.fromarray(a).save(f, "JPEG", quality=q, subsampling=s)` encodes with its defaults (JDCT_ISLOW,
the Annex K tables scaled by the quality, the four fixed Huffman tables, one interleaved scan, no restart intervals); all of that is
integer arithmetic, so the rule gives the file byte for byte (tests/test_jpeg_encode_rule_cpu.py: against Pillow itself and against
recorded files).

  encode_rule(rgb, quality, sampling)   uint8 [H, W, 3] -> the file's bytes
  scan_blocks(rgb, quality, sampling)   the quantised coefficients in scan order (`Blocks`): what the device's first launch leaves
  entropy_code(blocks)                  (`Coded`) the entropy-coded bytes and what the stream holds (stuffed bytes, ZRLs, ...)
  headers(W, H, quality, sampling)      the marker segments before the data; the device wrapper prepends the same bytes

The rule:
  colour        Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
                Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
  edges         per component wb = ceil(W h / (8 hmax)), hb = ceil(H v / (8 vmax)) blocks; the last column is replicated at full resolution
                out to wb 8 hmax / h columns, the last row at full resolution only up to a multiple of vmax / v; after downsampling the
                last *downsampled* row is replicated up to hb 8
  downsampling  h2v2 (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2, ... by output column; h2v1 (a + b + bias) >> 1, bias 0, 1, 0, 1, ...
  FDCT          jfdctint.c's "islow" on samples - 128: CONST_BITS 13, PASS1_BITS 2, rows then columns; its output is scaled by 8
  quantisation  sign(x) ((|x| + (q8 >> 1)) // q8), q8 = q << 3
  tables        Annex K; scale = 5000 // quality below 50, else 200 - 2 quality; entry = clip((base scale + 50) // 100, 1, 255)
  scan          MCUs in raster order, in an MCU the components in order, v rows of h blocks each; a block beyond wb or hb inside the last
                MCU column or row is a dummy: all AC zero, DC the quantised DC of the block before it in the MCU
  entropy       ITU T.81 F.1.2: DC differences per component, AC (run, size) codes, ZRL per 16 zeros, EOB only when the block ends in zeros;
                a negative value v is coded as v - 1 in its size's bits; bits MSB first, the last byte padded with ones, 00 after every FF
  file          SOI, APP0 JFIF 1.01 (units 0, density 1 x 1, no thumbnail), two DQT, SOF0 (component ids 1, 2, 3), four DHT (DC0, AC0, DC1,
                AC1), SOS, the data, EOI"""
import struct
from collections import namedtuple

import numpy as np

from .jpeg_rule import ZIGZAG, JpegRuleError

SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}            # luma (h, v); chroma is 1 x 1

# ITU T.81 Annex K.1 / K.2, natural (row-major) order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
                      100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32, np.int64)
# Annex K.3: (counts of the code lengths 1..16, values in code order); DC luminance, DC chrominance, AC luminance, AC chrominance
HUFF = {
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), bytes(range(12))),
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), bytes(range(12))),
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), bytes(
        [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
         0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
         0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
         0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
         0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
         0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
         0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])),
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), bytes(
        [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
         0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
         0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
         0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
         0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
         0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
         0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])),
}

# coef: int16 [blocks, 64], scan order, zig-zag order inside a block, DC absolute; comp: the component of every block; dummy: 0 a real
# block, 1 a dummy beyond the right edge, 2 a dummy beyond the bottom edge; geometry: (h, v, mcus_x, mcus_y, blocks per MCU)
Blocks = namedtuple("Blocks", "coef comp dummy geometry")
# data: the entropy-coded bytes with the stuffing; stuffed: 00s inserted; zrl: ZRL codes; no_eob: blocks whose 64th coefficient is not
# zero; max_ac_category / max_dc_category: the largest magnitude categories coded
Coded = namedtuple("Coded", "data stuffed zrl no_eob max_ac_category max_dc_category")


def quant_tables(quality):
    """(luminance, chrominance) int64 [64] in natural order for a quality of 1..100."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality={quality} (1..100)")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def code_table(counts, values):
    """{value: (code, length)} of a (counts, values) pair."""
    out, code, k = {}, 0, 0
    for length, n in enumerate(counts, 1):
        for _ in range(n):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def ycc(rgb):
    """int64 [3, H, W]."""
    r, g, b = (rgb[:, :, i].astype(np.int64) for i in range(3))
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                     (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16])


def _replicate(a, rows, cols):
    """`a` with its last row and column repeated out to [rows, cols]."""
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def component_plane(full, W, H, ch, cv, hmax, vmax):
    """A component's samples, padded to whole blocks: int64 [hb 8, wb 8] of its full-resolution plane [H, W]."""
    wb, hb = -(-W * ch // (8 * hmax)), -(-H * cv // (8 * vmax))
    fx, fy = hmax // ch, vmax // cv
    a = _replicate(full, -(-H // fy) * fy, wb * 8 * fx)
    if (fx, fy) == (2, 2):
        bias = 1 + (np.arange(a.shape[1] // 2) & 1)
        a = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + bias[None]) >> 2
    elif (fx, fy) == (2, 1):
        bias = np.arange(a.shape[1] // 2) & 1
        a = (a[:, 0::2] + a[:, 1::2] + bias[None]) >> 1
    elif (fx, fy) != (1, 1):
        raise ValueError(f"downsampling by {fx} x {fy}")
    return _replicate(a, hb * 8, wb * 8)


def _fdct_pass(d, first):
    """jfdctint.c's one-dimensional pass along axis 1 of int64 [n, 8, m]."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[:, i] for i in range(8))
    tmp0, tmp7, tmp1, tmp6, tmp2, tmp5, tmp3, tmp4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15

    def descale(x, s):
        return (x + (1 << (s - 1))) >> s

    o0, o4 = ((tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2) if first else (descale(tmp10 + tmp11, 2), descale(tmp10 - tmp11, 2))
    z1 = (tmp12 + tmp13) * 4433
    o2, o6 = descale(z1 + tmp13 * 6270, n), descale(z1 - tmp12 * 15137, n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o7, o5, o3, o1 = descale(tmp4 + z1 + z3, n), descale(tmp5 + z2 + z4, n), descale(tmp6 + z2 + z3, n), descale(tmp7 + z1 + z4, n)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=1)


def fdct_islow(samples):
    """int64 [n, 8, 8] (8 x scaled) of int64 [n, 8, 8] samples minus 128."""
    rows = _fdct_pass(samples.transpose(0, 2, 1), True).transpose(0, 2, 1)      # along a row: axis 2
    return _fdct_pass(rows, False)                                               # along a column: axis 1


def quantise(coef, q):
    """int64 [n, 64] of 8 x scaled coefficients [n, 64] and a table [64], both in natural order."""
    q8 = q.astype(np.int64)[None] << 3
    return np.sign(coef) * ((np.abs(coef) + (q8 >> 1)) // q8)


def scan_blocks(rgb, quality=90, sampling="420"):
    """`Blocks` of uint8 [H, W, 3]."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError(f"rgb: uint8 [H, W, 3], got {rgb.dtype} {tuple(rgb.shape)}")
    h, v = SAMPLINGS[sampling]
    H, W = rgb.shape[:2]
    tables = quant_tables(quality)
    mx, my = -(-W // (8 * h)), -(-H // (8 * v))
    per = h * v + 2
    planes = ycc(rgb)
    coef = np.zeros((my, mx, per, 64), np.int64)
    dummy = np.zeros((my, mx, per), np.uint8)
    comp = np.zeros((my, mx, per), np.uint8)
    first = 0
    for c in range(3):
        ch, cv = (h, v) if c == 0 else (1, 1)
        plane = component_plane(planes[c], W, H, ch, cv, h, v)
        hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
        blocks = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8) - 128
        q = quantise(fdct_islow(blocks).reshape(-1, 64), tables[0 if c == 0 else 1])[:, ZIGZAG].reshape(hb, wb, 64)
        grid = np.zeros((my * cv, mx * ch, 64), np.int64)
        grid[:hb, :wb] = q
        kind = np.zeros((my * cv, mx * ch), np.uint8)
        kind[:, wb:] = 1
        kind[hb:, :] = 2
        # [my cv, mx ch] -> [my, mx, cv ch]: v rows of h blocks
        coef[:, :, first:first + ch * cv] = grid.reshape(my, cv, mx, ch, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, ch * cv, 64)
        dummy[:, :, first:first + ch * cv] = kind.reshape(my, cv, mx, ch).transpose(0, 2, 1, 3).reshape(my, mx, ch * cv)
        comp[:, :, first:first + ch * cv] = c
        first += ch * cv
    for k in range(1, per):                                          # a dummy's DC: the block before it in the MCU (a chain, in order)
        coef[:, :, k, 0] = np.where(dummy[:, :, k] != 0, coef[:, :, k - 1, 0], coef[:, :, k, 0])
    return Blocks(coef.reshape(-1, 64).astype(np.int16), comp.reshape(-1), dummy.reshape(-1), (h, v, mx, my, per))


def entropy_code(blocks):
    """`Coded` of `Blocks`."""
    dc_t = [code_table(*HUFF[(0, 0)]), code_table(*HUFF[(0, 1)])]
    ac_t = [code_table(*HUFF[(1, 0)]), code_table(*HUFF[(1, 1)])]
    out = bytearray()
    acc = nacc = 0
    zrl = no_eob = max_ac = max_dc = 0
    pred = [0, 0, 0]
    for row, c in zip(blocks.coef.tolist(), blocks.comp.tolist()):
        t = 0 if c == 0 else 1
        diff = row[0] - pred[c]
        pred[c] = row[0]
        s = abs(diff).bit_length()
        if s > 11:
            raise JpegRuleError("DC category %d" % s)
        max_dc = max(max_dc, s)
        code, length = dc_t[t][s]
        acc = (((acc << length) | code) << s) | ((diff if diff >= 0 else diff - 1) & ((1 << s) - 1))
        nacc += length + s
        run = 0
        for x in row[1:]:
            if x == 0:
                run += 1
                continue
            while run > 15:
                code, length = ac_t[t][0xF0]
                acc = (acc << length) | code
                nacc += length
                run -= 16
                zrl += 1
            s = abs(x).bit_length()
            if s > 10:
                raise JpegRuleError("AC category %d" % s)
            max_ac = max(max_ac, s)
            code, length = ac_t[t][16 * run + s]
            acc = (((acc << length) | code) << s) | ((x if x >= 0 else x - 1) & ((1 << s) - 1))
            nacc += length + s
            run = 0
        if run:
            code, length = ac_t[t][0]
            acc = (acc << length) | code
            nacc += length
        else:
            no_eob += 1
        if nacc >= 8:                                                # whole bytes leave the accumulator
            keep = nacc & 7
            out += (acc >> keep).to_bytes(nacc >> 3, "big")
            acc &= (1 << keep) - 1
            nacc = keep
    if nacc:
        out.append(((acc << (8 - nacc)) | ((1 << (8 - nacc)) - 1)) & 0xFF)
    raw = bytes(out)
    return Coded(raw.replace(b"\xff", b"\xff\x00"), raw.count(b"\xff"), zrl, no_eob, max_ac, max_dc)


def _segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def headers(W, H, quality=90, sampling="420"):
    """The file's bytes from SOI to the end of the SOS header."""
    h, v = SAMPLINGS[sampling]
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError(f"size {W} x {H} (sides of 1 to 65535)")
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for tq, table in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes([tq]) + table[ZIGZAG].astype(np.uint8).tobytes())
    out += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 16 * h + v, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, th in ((0, 0), (1, 0), (0, 1), (1, 1)):
        counts, values = HUFF[(tc, th)]
        out += _segment(0xC4, bytes([16 * tc + th]) + bytes(counts) + values)
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode_rule(rgb, quality=90, sampling="420"):
    """The bytes of `Image.fromarray(rgb).save(f, "JPEG", quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[sampling])`."""
    rgb = np.asarray(rgb)
    blocks = scan_blocks(rgb, quality, sampling)
    return headers(rgb.shape[1], rgb.shape[0], quality, sampling) + entropy_code(blocks).data + b"\xff\xd9"
