"""The corpus of the device JPEG decoder, generated from seeds through Pillow's encoder (libjpeg-turbo).  Shared by
tests/test_jpeg_rule_cpu.py, test_jpeg_entropy_cpu.py, test_jpeg_decode_gpu.py, test_jpeg_mapper_gpu.py and tools/gen_golden_jpeg.py.

  covered_cases()     files the device decoder takes: five sizes x four samplings, content (smooth, noise, flat saturated patches) and
                      quality (5, 30, 75, 90, 100) cycled so that every value of each meets every sampling; optimize=True (custom Huffman
                      tables); restart markers every 3 blocks and every MCU row; the chunk-crossing file
  uncovered_files()   progressive, CMYK, EXIF-rotated, 4 x 4: they decode through the fallback
  malformed_files()   truncations, a flipped bit in the entropy data, a Huffman table with a count overflow, a frame header that announces
                      more blocks than the data holds, a DRI that disagrees with the markers
"""
import functools
import io
import struct
from collections import namedtuple

import numpy as np
from PIL import Image

Case = namedtuple("Case", "name data")

SIZES = ((16, 16), (17, 31), (40, 48), (75, 131), (200, 264))        # (H, W)
SAMPLINGS = ("444", "422", "420", "grey")
CONTENTS = ("smooth", "noise", "patches")
QUALITIES = (5, 30, 75, 90, 100)
_SUB = {"444": 0, "422": 1, "420": 2}


def content(kind, H, W, seed):
    """uint8 [H, W, 3]."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "smooth":
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        f = rng.uniform(0.02, 0.2, (3, 2))
        ph = rng.uniform(0, 6.28, 3)
        a = np.stack([127.5 + 127.5 * np.sin(f[c, 0] * y + f[c, 1] * x + ph[c]) for c in range(3)], axis=2)
        return np.clip(a + rng.normal(0, 2, a.shape), 0, 255).astype(np.uint8)
    # flat patches of saturated colours: they push the clamp of the colour conversion
    corners = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
    a = np.zeros((H, W, 3), np.uint8)
    step = max(3, min(H, W) // 4)
    for y0 in range(0, H, step):
        for x0 in range(0, W, step + 2):
            a[y0:y0 + step, x0:x0 + step + 2] = corners[rng.integers(0, 8)]
    return a


def encode(a, sampling, quality, **kw):
    buf = io.BytesIO()
    if sampling == "grey":
        Image.fromarray(a[:, :, 1]).save(buf, format="JPEG", quality=quality, **kw)
    else:
        Image.fromarray(a).save(buf, format="JPEG", quality=quality, subsampling=_SUB[sampling], **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def covered_cases():
    out = []
    k = 0
    for si, (H, W) in enumerate(SIZES):
        for sj, sampling in enumerate(SAMPLINGS):
            # two files per (size, sampling); over the table every content and every quality meets every sampling
            for rep in range(2):
                kind = CONTENTS[(si + sj + rep) % 3]
                quality = QUALITIES[(si + 2 * sj + 3 * rep) % 5]
                if (H, W) == (200, 264) and rep == 1:
                    continue                                         # (one file of the large size per sampling)
                out.append(Case(f"{kind}_{H}x{W}_{sampling}_q{quality}", encode(content(kind, H, W, 100 + k), sampling, quality)))
                k += 1
    for sampling in SAMPLINGS:
        a = content("noise", 40, 48, 300 + len(out))
        out.append(Case(f"optimize_40x48_{sampling}_q75", encode(a, sampling, 75, optimize=True)))
        a = content("smooth", 75, 131, 400 + len(out))
        out.append(Case(f"restart3_75x131_{sampling}_q90", encode(a, sampling, 90, restart_marker_blocks=3)))
        a = content("patches", 75, 131, 500 + len(out))
        out.append(Case(f"restartrow_75x131_{sampling}_q30", encode(a, sampling, 30, restart_marker_rows=1)))
    out.append(Case("restart3_optimize_17x31_420_q100", encode(content("noise", 17, 31, 7), "420", 100, optimize=True, restart_marker_blocks=3)))
    out.append(chunk_crossing())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chunk_crossing():
    """Noise at quality 100, 4:4:4, one interval: more than 1024 subsequences of 32 bits and of 64 bits, so the synchronisation loop of
    a 1024-lane workgroup crosses a chunk boundary at both."""
    return Case("chunk_crossing_64x72_444_q100", encode(content("noise", 64, 72, 11), "444", 100))


def same_size_batch():
    """Files of one size (75 x 131, 4:2:0), with and without restart markers: the mixed batch."""
    return tuple(c for c in covered_cases() if "75x131_420" in c.name)


def frames(n=5, H=75, W=131, sampling="420", quality=90, seed=900):
    """n files of one size, as a video's frames."""
    return [encode(content("smooth", H, W, seed + i), sampling, quality) for i in range(n)]


def pillow_pixels(data):
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


# ---- not covered ----------------------------------------------------------------------------------------------------------------------------
def _with_exif_orientation(data, orientation):
    exif = Image.Exif()
    exif[274] = orientation
    buf = io.BytesIO()
    with Image.open(io.BytesIO(data)) as im:
        im.save(buf, format="JPEG", quality=90, exif=exif.tobytes())
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def uncovered_files():
    a = content("smooth", 40, 48, 21)
    cmyk = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(cmyk, format="JPEG", quality=90)
    return {"progressive": encode(a, "420", 75, progressive=True),
            "cmyk": cmyk.getvalue(),
            "exif rotated": _with_exif_orientation(encode(a, "444", 90), 6),
            "4x4": encode(content("noise", 4, 4, 22), "420", 90)}


UNCOVERED_REASONS = {"progressive": "progressive", "cmyk": "colour: 4 components", "exif rotated": "EXIF orientation 6",
                     "4x4": "size 4 x 4 (sides of 16 to 16384)"}


# ---- malformed ------------------------------------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, offset of the FF, offset past the segment)] up to and including SOS."""
    pos, out = 2, []
    while True:
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((m, pos, pos + 2 + n))
        pos += 2 + n
        if m == 0xDA:
            return out


def entropy_start(data):
    return segments(data)[-1][2]


@functools.lru_cache(maxsize=None)
def malformed_files():
    """{name: bytes}.  Built from two small covered files, one without and one with restart markers."""
    plain = encode(content("noise", 40, 48, 31), "420", 90)
    rst = encode(content("noise", 40, 48, 32), "420", 90, restart_marker_blocks=3)
    e0 = entropy_start(plain)
    out = {}
    for name, cut in (("truncated in the headers", e0 - 5), ("truncated at the first entropy byte", e0 + 1),
                      ("truncated in the middle", (e0 + len(plain)) // 2), ("truncated before EOI", len(plain) - 2),
                      ("truncated in the last bytes", len(plain) - 6)):
        out[name] = plain[:cut]
    mid = (e0 + len(plain)) // 2
    while plain[mid] in (0xFF, 0x00) or plain[mid - 1] == 0xFF or (plain[mid] ^ 0x10) == 0xFF:
        mid += 1
    out["flipped bit"] = plain[:mid] + bytes([plain[mid] ^ 0x10]) + plain[mid + 1:]
    # a Huffman table whose counts over-subscribe length 1 (three codes of one bit)
    dht = next(s for s in segments(plain) if s[0] == 0xC4)
    out["huffman count overflow"] = plain[:dht[1] + 5] + bytes([3]) + plain[dht[1] + 6:]
    # a frame header 16 rows taller than the data
    sof = next(s for s in segments(plain) if s[0] == 0xC0)
    out["more blocks than data"] = plain[:sof[1] + 5] + struct.pack(">H", 40 + 32) + plain[sof[1] + 7:]
    # DRI against the markers: the interval doubled, and a file with markers whose DRI says none
    dri = next(s for s in segments(rst) if s[0] == 0xDD)
    ri = struct.unpack(">H", rst[dri[1] + 4:dri[1] + 6])[0]
    out["dri doubled"] = rst[:dri[1] + 4] + struct.pack(">H", 2 * ri) + rst[dri[1] + 6:]
    out["dri removed"] = rst[:dri[1]] + rst[dri[2]:]
    return out


def host_read(data):
    """What the host reader does with a file's bytes: ("pixels", array) or ("raises", exception type)."""
    try:
        return "pixels", pillow_pixels(data)
    except Exception as e:                                           # noqa: BLE001 (whatever Pillow raises is the behaviour to keep)
        return "raises", type(e)


# ---- a hand-built file whose dequantised coefficients leave int16 ------------------------------------------------------------------------------
def oversized_product():
    """A covered 16 x 16 grey file, quantisation table all 255, whose first block has a DC of 1020: 255 x 1020 > 32767."""
    base = encode(content("smooth", 16, 16, 41), "grey", 50)
    segs = segments(base)
    dqt = next(s for s in segs if s[0] == 0xDB)
    body = bytearray(base)
    body[dqt[1] + 5:dqt[1] + 5 + 64] = bytes([255]) * 64
    # standard luminance DC table: category 10 has the code 11111110 (8 bits); then 10 bits of magnitude; every block ends with EOB of the
    # standard AC table (1010); the three other blocks have a DC difference of category 0 (00) and EOB
    bits = "11111110" + format(1020, "010b") + "1010" + ("00" + "1010") * 3
    bits += "1" * (-len(bits) % 8)
    ecs = int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
    return bytes(body[:segs[-1][2]]) + ecs + b"\xff\xd9"
