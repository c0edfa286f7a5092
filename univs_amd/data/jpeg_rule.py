"""Baseline JPEG as Pillow decodes it, stated once in numpy: the yardstick of csrc/jpeg_decode.hip, in the role inference/png_rule.py has
for the PNG encoder.  No GPU.

Pillow links libjpeg-turbo and decodes with its defaults (JDCT_ISLOW, fancy upsampling, no draft mode); all of that is integer
arithmetic, so the rule gives `np.asarray(Image.open(f).convert("RGB"))` byte for byte (tests/test_jpeg_rule_cpu.py: against Pillow itself
and against recorded bytes).

  parse_jpeg(data)   the marker segments up to SOS -> `Parsed`; `status` is "ok" or says what stopped the walk
  covered(parsed)    whether the device decoder takes the file; why_uncovered(parsed) says why not
  decode_rule(data)  the serial decoder -> `Decoded` (pixels, coefficient blocks in natural order with absolute DC, in_range)

The rule:
  entropy     ITU T.81 F.2.2: per block a DC category + difference, then (run, size) pairs in zig-zag order; EOB, ZRL; stuffed 00 after FF
              removed; at RSTn the bit reader realigns and the DC predictors return to 0
  dequantise  coef * q in natural order
  IDCT        jidctint.c's 8 x 8 "islow": CONST_BITS 13, PASS1_BITS 2; columns first, descaled by 11, then rows, descaled by 18;
              DESCALE(x, n) = (x + (1 << (n - 1))) >> n with an arithmetic shift; output clamp(x + 128, 0, 255)
  upsampling  "fancy" (triangle), on the component's downsampled extent ceil(W h / hmax) x ceil(H v / vmax) with edge samples replicated:
              h2v1 left (3 c + l + 1) >> 2, right (3 c + r + 2) >> 2; h2v2 column sums 3 cur + above (upper row) / 3 cur + below (lower row),
              then left (3 s + s_l + 8) >> 4, right (3 s + s_r + 7) >> 4
  colour      R = y + ((91881 cr + 32768) >> 16), B = y + ((116130 cb + 32768) >> 16), G = y + ((-22554 cb - 46802 cr + 32768) >> 16)
              with cb, cr minus 128, each clamped; one component: the three channels equal

libjpeg-turbo's SIMD and C code agree only inside a range (16-bit products, a saturating pack after the first pass, a masked range-limit
table), so `in_range` is False when any |coef q| > 32767, a first-pass output leaves int16 or a second-pass value before the clamp leaves
[-512, 511]: such a file goes to Pillow.  libjpeg-turbo replicates chroma instead of interpolating when a chroma plane has one or two
columns; `covered` keeps those files (W < 16 or H < 16) with Pillow."""
from collections import namedtuple

import numpy as np

# zig-zag index -> natural (row-major) index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
                  np.int64)
MIN_SIDE = 16                                                        # below it Pillow decodes (one- and two-column chroma planes)
MAX_SIDE = 16384

# components: ((id, h, v, tq), ...); scan: ((component index, td, ta), ...) in scan order; quant: {tq: (precision bit, uint16 [64] natural order)};
# huff: {(class, id): (counts [16], values bytes)}; ecs: (first byte of the entropy-coded data, len(data)): the device finds the end
# of the data itself, at the first marker that is no RSTn; colour: "grey", "ycc" or what libjpeg would take the components for
Parsed = namedtuple("Parsed", "status width height precision sof components scan quant huff restart_interval ecs orientation colour data")
Decoded = namedtuple("Decoded", "pixels blocks in_range")


class JpegRuleError(ValueError):
    """The entropy-coded data breaks a rule (`decode_rule`); the message names it."""


def _fail(status, data, **kw):
    base = dict(status=status, width=0, height=0, precision=0, sof=None, components=(), scan=(), quant={}, huff={}, restart_interval=0,
                ecs=(0, 0), orientation=None, colour=None, data=data)
    base.update(kw)
    return Parsed(**base)


def huffman_ok(counts, nvalues):
    """A (counts, values) pair is a usable code: the values are all there, at most 256, and no length is over-subscribed."""
    if sum(counts) != nvalues or nvalues > 256:
        return False
    code = 0
    for length, n in enumerate(counts, 1):
        code += n
        if code > (1 << length):
            return False
        code <<= 1
    return True


def _orientation(data):
    """The EXIF orientation through Pillow's lazy open (no pixel is decoded); None where it has none or the block does not parse."""
    import io
    from PIL import Image
    try:
        with Image.open(io.BytesIO(data)) as im:
            return im.getexif().get(274)
    except Exception:
        return None


def parse_jpeg(data):
    """`Parsed` of a file's bytes: the walk over the marker segments up to and including the SOS header.  Never raises on bytes:
    `status` is "ok", or "not a JPEG file", "truncated in the headers", "bad <segment>", "no frame header before the scan", ... and
    the fields read so far."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return _fail("not a JPEG file", data)
    pos = 2
    got = dict(quant={}, huff={}, restart_interval=0, orientation=None)
    frame = None
    jfif = adobe = None
    has_exif = False
    while True:
        if pos + 4 > n:
            return _fail("truncated in the headers", data, **got)
        if data[pos] != 0xFF:
            return _fail("bytes that are no marker between the segments", data, **got)
        m = data[pos + 1]
        if m == 0xFF:                                                # a fill byte
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:                           # markers without a segment
            pos += 2
            continue
        if m == 0xD9:
            return _fail("end of image before a scan", data, **got)
        length = (data[pos + 2] << 8) | data[pos + 3]
        if length < 2 or pos + 2 + length > n:
            return _fail("truncated in the headers", data, **got)
        seg = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if m == 0xDB:                                                # DQT
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                size = 64 * (2 if pq else 1)
                if pq > 1 or tq > 3 or q + 1 + size > len(seg):
                    return _fail("bad DQT", data, **got)
                raw = np.frombuffer(seg, np.uint8 if pq == 0 else ">u2", 64, q + 1).astype(np.uint16)
                nat = np.zeros(64, np.uint16)
                nat[ZIGZAG] = raw
                got["quant"][tq] = (pq, nat)
                q += 1 + size
        elif m == 0xC4:                                              # DHT
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    return _fail("bad DHT", data, **got)
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = tuple(seg[q + 1:q + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or q + 17 + total > len(seg) or not huffman_ok(counts, total):
                    return _fail("bad DHT", data, **got)
                got["huff"][(tc, th)] = (counts, bytes(seg[q + 17:q + 17 + total]))
                q += 17 + total
        elif m == 0xDD:                                              # DRI
            if len(seg) != 2:
                return _fail("bad DRI", data, **got)
            got["restart_interval"] = (seg[0] << 8) | seg[1]
        elif 0xC0 <= m <= 0xCF and m not in (0xC8, 0xCC):            # SOFn (0xC4 and 0xCC are handled above / below)
            if frame is not None:
                return _fail("two frame headers", data, **got)
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                return _fail("bad SOF", data, **got)
            comps = tuple((seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5]))
            frame = dict(sof=m - 0xC0, precision=seg[0], height=(seg[1] << 8) | seg[2], width=(seg[3] << 8) | seg[4], components=comps)
        elif m == 0xCC:
            return _fail("arithmetic conditioning table", data, **got, **(frame or {}))
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xE1 and seg[:6] == b"Exif\0\0":
            has_exif = True
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDA:                                              # SOS: the walk ends here
            if frame is None:
                return _fail("no frame header before the scan", data, **got)
            if len(seg) < 1 or len(seg) != 1 + 2 * seg[0] + 3:
                return _fail("bad SOS", data, **got, **frame)
            ids = [c[0] for c in frame["components"]]
            scan = []
            for i in range(seg[0]):
                cid, t = seg[1 + 2 * i], seg[2 + 2 * i]
                if cid not in ids or ids.index(cid) in [s[0] for s in scan]:
                    return _fail("bad SOS", data, **got, **frame)
                scan.append((ids.index(cid), t >> 4, t & 15))
            ncomp = len(ids)
            if ncomp == 1:
                colour = "grey"
            elif ncomp == 3:                                         # libjpeg's default_decompress_parms
                if jfif:
                    colour = "ycc"
                elif adobe is not None:
                    colour = {0: "rgb", 1: "ycc"}.get(adobe, "adobe transform %d" % adobe)
                else:
                    colour = "rgb" if ids == [82, 71, 66] else "ycc"
            else:
                colour = "%d components" % ncomp
            if has_exif:
                got["orientation"] = _orientation(data)
            spectral = tuple(seg[1 + 2 * seg[0]:])
            return Parsed(status="ok", scan=tuple(scan) + (("spectral",) + spectral,), ecs=(pos, n), colour=colour, data=data, **got, **frame)
        # every other segment (APPn, COM, ...) is skipped


def why_uncovered(p):
    """None for a file the device decoder takes, else the reason in words."""
    if p.status != "ok":
        return p.status
    if p.sof not in (0, 1):
        return {2: "progressive"}.get(p.sof, "SOF%d" % p.sof)
    if p.precision != 8:
        return "%d-bit samples" % p.precision
    if p.colour not in ("grey", "ycc"):
        return "colour: " + str(p.colour)
    scan, spectral = p.scan[:-1], p.scan[-1][1:]
    if len(scan) != len(p.components) or [s[0] for s in scan] != list(range(len(scan))):
        return "no single scan holding all components in frame order"
    if spectral != (0, 63, 0):
        return "spectral selection in a sequential scan"
    if p.orientation not in (None, 1):
        return "EXIF orientation %r" % (p.orientation,)
    if not (MIN_SIDE <= p.width <= MAX_SIDE and MIN_SIDE <= p.height <= MAX_SIDE):
        return "size %d x %d (sides of %d to %d)" % (p.width, p.height, MIN_SIDE, MAX_SIDE)
    for k, (cid, h, v, tq) in enumerate(p.components):
        if tq not in p.quant:
            return "component %d: no quantisation table %d" % (k, tq)
        if p.quant[tq][0] != 0:
            return "16-bit quantisation table"
        if (0, scan[k][1]) not in p.huff or (1, scan[k][2]) not in p.huff:
            return "component %d: no Huffman table" % k
    if len(p.components) == 3:
        (_, h0, v0, _), (_, h1, v1, _), (_, h2, v2, _) = p.components
        if (h1, v1, h2, v2) != (1, 1, 1, 1) or (h0, v0) not in ((1, 1), (2, 1), (2, 2)):
            return "sampling %dx%d %dx%d %dx%d" % (h0, v0, h1, v1, h2, v2)
    return None


def covered(p):
    return why_uncovered(p) is None


def geometry(p):
    """(h, v, mcus_x, mcus_y, blocks per MCU, component of each block of an MCU) of a covered file; one component is h = v = 1
    whatever the frame header says (a scan of one component is not interleaved)."""
    if len(p.components) == 1:
        h = v = 1
        order = (0,)
    else:
        h, v = p.components[0][1], p.components[0][2]
        order = (0,) * (h * v) + (1, 2)
    mx, my = -(-p.width // (8 * h)), -(-p.height // (8 * v))
    return h, v, mx, my, len(order), order


def unstuff(data, start):
    """(intervals [bytes], status): the entropy-coded data from `start` without the stuffed 00s, cut at the RSTn markers, up to the
    first other marker; status "ok", "restart markers out of sequence" or "no end-of-image marker after the data" (the marker that
    ends the data has to be EOI: the host reader refuses a file without one)."""
    a = np.frombuffer(data, np.uint8, len(data) - start, start)
    nxt = np.append(a[1:], 0xD9)                                    # (a last FF ends the data)
    prv = np.append(0, a[:-1])
    ff = a == 0xFF
    rst = ff & (nxt >= 0xD0) & (nxt <= 0xD7)
    end = ff & ~rst & (nxt != 0) & (nxt != 0xFF)
    stop = int(np.argmax(end)) if end.any() else len(a)
    keep = ((~ff) & (prv != 0xFF)) | (ff & (nxt == 0))
    keep[stop:] = False
    cuts = np.flatnonzero(rst[:stop])
    status = "ok" if np.array_equal(nxt[cuts] - 0xD0, np.arange(len(cuts)) % 8) else "restart markers out of sequence"
    if stop + 1 >= len(a) or a[stop + 1] != 0xD9:
        status = "no end-of-image marker after the data"
    out, lo = [], 0
    for c in list(cuts) + [stop]:
        out.append(a[lo:c][keep[lo:c]].tobytes())
        lo = c
    return out, status


def _lut(counts, values):
    """16-bit look-ahead -> (length, value); length 0 where the bits are no code."""
    length = np.zeros(65536, np.uint8)
    value = np.zeros(65536, np.uint8)
    code, k = 0, 0
    for l, n in enumerate(counts, 1):
        for _ in range(n):
            lo = code << (16 - l)
            length[lo:lo + (1 << (16 - l))] = l
            value[lo:lo + (1 << (16 - l))] = values[k]
            code += 1
            k += 1
        code <<= 1
    return length.tolist(), value.tolist()


def decode_blocks(p):
    """int16 [blocks, 64] of a covered file in scan order, natural order inside a block, DC absolute.  Raises JpegRuleError."""
    h, v, mx, my, per, order = geometry(p)
    scan = p.scan[:-1]
    luts = {key: _lut(*tab) for key, tab in p.huff.items()}
    dc_l = [luts[(0, scan[c][1])] for c in range(len(scan))]
    ac_l = [luts[(1, scan[c][2])] for c in range(len(scan))]
    mcus = mx * my
    ri = p.restart_interval or mcus
    intervals, status = unstuff(p.data, p.ecs[0])
    if status != "ok":
        raise JpegRuleError(status)
    if len(intervals) != -(-mcus // ri):
        raise JpegRuleError("%d restart intervals, the frame has %d" % (len(intervals), -(-mcus // ri)))
    blocks = np.zeros((mcus * per, 64), np.int16)
    zz = ZIGZAG.tolist()
    nb = 0
    for k, raw in enumerate(intervals):
        total = 8 * len(raw)
        raw += bytes(8)
        frm = int.from_bytes
        pos = 0
        pred = [0, 0, 0]
        for _ in range(min(ri, mcus - k * ri) * per):
            c = order[nb % per]
            row = [0] * 64
            z = 0
            while z < 64:
                if pos >= total:
                    raise JpegRuleError("data exhausted before the expected number of blocks")
                i = pos >> 3
                look = (frm(raw[i:i + 3], "big") >> (8 - (pos & 7))) & 0xFFFF
                ln, val = dc_l[c] if z == 0 else ac_l[c]
                l = ln[look]
                if l == 0:
                    raise JpegRuleError("invalid code")
                pos += l
                sym = val[look]
                if z == 0:
                    s, r = sym, 0
                    if s > 11:
                        raise JpegRuleError("DC category %d" % s)
                else:
                    r, s = sym >> 4, sym & 15
                    if s == 0:
                        if r != 15:
                            z = 64
                            break
                        z += 16
                        if z > 64:
                            raise JpegRuleError("a run past the end of the block")
                        continue
                    if s > 10:
                        raise JpegRuleError("AC category %d" % s)
                    z += r
                    if z > 63:
                        raise JpegRuleError("a run past the end of the block")
                i = pos >> 3
                x = (frm(raw[i:i + 3], "big") >> (24 - (pos & 7) - s)) & ((1 << s) - 1) if s else 0
                pos += s
                if s and x < (1 << (s - 1)):
                    x -= (1 << s) - 1
                if pos > total:
                    raise JpegRuleError("data exhausted before the expected number of blocks")
                if z == 0:
                    pred[c] += x
                    if not -32768 <= pred[c] <= 32767:
                        raise JpegRuleError("DC outside int16")
                    row[0] = pred[c]
                else:
                    row[zz[z]] = x
                z += 1
            blocks[nb] = row
            nb += 1
    return blocks


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(c, shift):
    """jidctint.c's one-dimensional pass along axis 1 of int64 [n, 8, m]."""
    c0, c1, c2, c3, c4, c5, c6, c7 = (c[:, i] for i in range(8))
    z1 = (c2 + c6) * 4433
    tmp2 = z1 - c6 * 15137
    tmp3 = z1 + c2 * 6270
    tmp0 = (c0 + c4) << 13
    tmp1 = (c0 - c4) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    o0, o1, o2, o3 = c7, c5, c3, c1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([_descale(x, shift) for x in out], axis=1)


def idct_islow(coef, q):
    """(uint8 [n, 8, 8], in_range) of int16 [n, 64] coefficient blocks and a uint16 [64] table, both in natural order."""
    d = coef.astype(np.int64) * q.astype(np.int64)[None]
    ok = bool((np.abs(d) <= 32767).all())
    ws = _pass(d.reshape(-1, 8, 8), 11)                              # columns: axis 1 is the row index
    ok = ok and bool(((ws >= -32768) & (ws <= 32767)).all())
    px = _pass(ws.transpose(0, 2, 1), 18).transpose(0, 2, 1)         # rows
    ok = ok and bool(((px >= -512) & (px <= 511)).all())
    return np.clip(px + 128, 0, 255).astype(np.uint8), ok


def planes_from_blocks(p, blocks):
    """([uint8 plane per component, padded to whole MCUs], in_range)."""
    h, v, mx, my, per, order = geometry(p)
    b = blocks.reshape(my, mx, per, 64)
    planes, ok = [], True
    for c in range(len(p.components)):
        ch, cv = (h, v) if c == 0 else (1, 1)
        first = 0 if c == 0 else h * v + c - 1
        px, good = idct_islow(b[:, :, first:first + ch * cv].reshape(-1, 64), p.quant[p.components[c][3]][1])
        ok = ok and good
        px = px.reshape(my, mx, cv, ch, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * cv * 8, mx * ch * 8)
        planes.append(px)
    return planes, ok


def _clamp_take(a, idx, axis):
    return np.take(a, np.clip(idx, 0, a.shape[axis] - 1), axis=axis)


def upsample_h2(c):
    """h2v1 fancy upsampling of int64 [rows, cols] -> [rows, 2 cols]."""
    x = np.arange(c.shape[1])
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + _clamp_take(c, x - 1, 1) + 1) >> 2
    out[:, 1::2] = (3 * c + _clamp_take(c, x + 1, 1) + 2) >> 2
    return out


def upsample_h2v2(c):
    """h2v2 fancy upsampling of int64 [rows, cols] -> [2 rows, 2 cols]."""
    y, x = np.arange(c.shape[0]), np.arange(c.shape[1])
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int64)
    for half, dy in ((0, -1), (1, 1)):
        s = 3 * c + _clamp_take(c, y + dy, 0)
        out[half::2, 0::2] = (3 * s + _clamp_take(s, x - 1, 1) + 8) >> 4
        out[half::2, 1::2] = (3 * s + _clamp_take(s, x + 1, 1) + 7) >> 4
    return out


def pixels_from_planes(p, planes):
    """uint8 [H, W, 3]."""
    H, W = p.height, p.width
    h, v = geometry(p)[:2]
    y = planes[0][:H, :W].astype(np.int64)
    if len(planes) == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    dh, dw = -(-H // v), -(-W // h)
    chroma = []
    for c in (1, 2):
        a = planes[c][:dh, :dw].astype(np.int64)
        if (h, v) == (2, 1):
            a = upsample_h2(a)
        elif (h, v) == (2, 2):
            a = upsample_h2v2(a)
        chroma.append(a[:H, :W] - 128)
    cb, cr = chroma
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode_rule(data):
    """`Decoded` of a covered file's bytes.  Raises ValueError for a file that is not covered (with the reason) and JpegRuleError where
    the entropy-coded data breaks a rule."""
    p = data if isinstance(data, Parsed) else parse_jpeg(data)
    why = why_uncovered(p)
    if why is not None:
        raise ValueError("decode_rule: not covered: " + why)
    blocks = decode_blocks(p)
    planes, ok = planes_from_blocks(p, blocks)
    return Decoded(pixels_from_planes(p, planes), blocks, ok)


def table_bytes(p):
    """The Huffman tables of a covered file as the device takes them: uint8 [2 components, 272], row 2 c the DC and row 2 c + 1 the AC
    table of component c, each 16 counts and the values padded with zeros to 256."""
    out = np.zeros((2 * len(p.components), 272), np.uint8)
    for c, (_, td, ta) in enumerate(p.scan[:-1]):
        for k, key in enumerate(((0, td), (1, ta))):
            counts, values = p.huff[key]
            out[2 * c + k, :16] = counts
            out[2 * c + k, 16:16 + len(values)] = np.frombuffer(values, np.uint8)
    return out
