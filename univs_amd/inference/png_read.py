"""The container of a PNG file, parsed on the host for the device reader (png_read_ops.py, csrc/png_inflate.hip).

  parse_png   signature, chunks, IHDR, PLTE, the concatenated IDAT payloads; the CRC of the critical chunks
  covered     what the device reads; everything else goes to Pillow as before

The host reads a few dozen bytes of headers per file; the zlib stream is uploaded as it is.  Ancillary chunks are skipped, `tRNS`
included: `np.array(im)` of a mode-P image returns the indices with or without it.  Any parse error is a `PngParseError`, and the
caller hands that file to Pillow, so the exception a user sees is the one they see today.
"""
import struct
import zlib
from collections import namedtuple

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_ROWBYTES = 24576          # csrc/png_inflate_core.h: PNG_ROW_CAP, the row kept in LDS; 8191 RGB pixels fit
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}

# width, height, bit_depth, colour_type, compression, filter_method, interlace: the IHDR; palette: the PLTE payload or None;
# idat: the zlib stream (every IDAT payload, concatenated)
PngInfo = namedtuple("PngInfo", "width height bit_depth colour_type compression filter_method interlace palette idat")


class PngParseError(ValueError):
    pass


def parse_png(data):
    """`PngInfo` of the file `data` (bytes).  PngParseError: a bad signature, a truncated chunk, a CRC mismatch in a critical chunk, a
    missing IHDR / IDAT / IEND, IHDR not first or not 13 bytes, a PLTE that is no multiple of 3 or longer than 768, a palette image
    without PLTE."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise PngParseError("bad signature")
    pos, header, palette, idat, ended = 8, None, None, [], False
    while pos < len(data):
        if pos + 8 > len(data):
            raise PngParseError("truncated chunk header")
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + length > len(data):
            raise PngParseError(f"truncated {kind!r} chunk")
        payload = data[pos + 8:pos + 8 + length]
        critical = not kind[0] & 0x20
        if critical and zlib.crc32(kind + payload) != struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])[0]:
            raise PngParseError(f"CRC mismatch in {kind!r}")
        pos += 12 + length
        if header is None and kind != b"IHDR":
            raise PngParseError("IHDR is not the first chunk")
        if kind == b"IHDR":
            if header is not None or length != 13:
                raise PngParseError("bad IHDR")
            header = struct.unpack(">IIBBBBB", payload)
        elif kind == b"PLTE":
            if length % 3 or not 0 < length <= 768:
                raise PngParseError("bad PLTE")
            palette = payload
        elif kind == b"IDAT":
            idat.append(payload)
        elif kind == b"IEND":
            ended = True
            break
        elif critical:
            raise PngParseError(f"unknown critical chunk {kind!r}")
    if header is None or not idat or not ended:
        raise PngParseError("missing IHDR, IDAT or IEND")
    if header[3] == 3 and palette is None:
        raise PngParseError("palette image without PLTE")
    return PngInfo(*header, palette, b"".join(idat))


def rowbytes(info):
    """Bytes of a row after its filter byte."""
    return (info.width * CHANNELS[info.colour_type] * info.bit_depth + 7) // 8


def covered(info):
    """True where the device reads the file (include/univs_pngread_hip.h): non-interlaced, compression and filter method 0, colour type
    0 or 2 at bit depth 8 or colour type 3 at bit depth 1, 2, 4 or 8, W, H >= 1, a row of at most MAX_ROWBYTES bytes and fewer than 2^31
    filtered and output bytes."""
    if info.interlace != 0 or info.compression != 0 or info.filter_method != 0:
        return False
    if not ((info.colour_type in (0, 2) and info.bit_depth == 8) or (info.colour_type == 3 and info.bit_depth in (1, 2, 4, 8))):
        return False
    if info.width < 1 or info.height < 1 or rowbytes(info) > MAX_ROWBYTES:
        return False
    return info.height * (1 + rowbytes(info)) < 2 ** 31 and info.height * info.width * 3 < 2 ** 31


def why_uncovered(info):
    """One phrase for `uncovered="raise"`."""
    if info.interlace != 0:
        return "interlaced"
    if info.compression != 0 or info.filter_method != 0:
        return f"compression method {info.compression}, filter method {info.filter_method}"
    if not covered(info._replace(width=1, height=1)):
        return f"colour type {info.colour_type} at bit depth {info.bit_depth}"
    return f"size {info.width} x {info.height}"
