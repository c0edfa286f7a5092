// The serial half of the PNG reader (include/univs_pngread_hip.h), as plain C++ for the host and the device: the frame plan, the bit
// reader, the Huffman table builder, the symbol decoder, every bounds decision of RFC 1950 / 1951 inflate and the status enum.  The
// lane-parallel half is the template parameter `L`:
//
//   L::N        lanes that share one stream (64 on the device: one wave; 1 in tools/png_inflate_host.cpp)
//   L::lane()   this lane, in [0, N)
//   L::sync()   orders the stores of all lanes before the loads of all lanes that follow (a barrier on the device, nothing on the host)
//
// Every lane runs the serial text on the same values, so every branch is uniform; only the literal store (lane 0), the match and
// stored-block copies (lane j takes the bytes j, j + N, ...) and the Adler partial sums differ between lanes.
//
// The rules this file keeps for untrusted bytes:
//   * every loop is counted by input bits consumed or output bytes produced: a block takes at least 3 bits, a symbol at least 1;
//   * a load of `in` happens only at pos in [in_begin, in_end), a store to `out` only at n in [0, expect), the ring is indexed & 32767,
//     the tables by a decoded index below the number of coded symbols;
//   * the first violated rule ends the stream with its status; nothing is retried.
// Accepted is what zlib's inflate accepts: an incomplete code only where it is a single code of one bit (or no distance code at all).
#ifndef UNIVS_PNG_INFLATE_CORE_H
#define UNIVS_PNG_INFLATE_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

namespace univs {

// status[f] of univs_png_read (include/univs_pngread_hip.h documents the values; tests pin them)
enum PngStatus {
  PNG_OK = 0,
  PNG_ERR_DESC = 1,          // the descriptor or the frame's offsets: sizes, colour type / bit depth / channels, palette row, regions
  PNG_ERR_ZLIB_HEADER = 2,   // CM != 8, window > 32 KB, FCHECK, preset dictionary
  PNG_ERR_INPUT = 3,         // input exhausted
  PNG_ERR_BLOCK_TYPE = 4,    // block type 3
  PNG_ERR_STORED_LEN = 5,    // LEN != ~NLEN
  PNG_ERR_CODE_LENGTHS = 6,  // over-subscribed or forbidden incomplete code, HLIT > 286, HDIST > 30, no end-of-block code
  PNG_ERR_REPEAT = 7,        // repeat code without a previous length, or beyond the lengths of the block
  PNG_ERR_SYMBOL = 8,        // literal/length 286 / 287, distance code 30 / 31, bits that are no code of an incomplete table
  PNG_ERR_DISTANCE = 9,      // a distance beyond the bytes produced
  PNG_ERR_OVERFLOW = 10,     // more than H (1 + rowbytes) bytes
  PNG_ERR_SHORT = 11,        // fewer at the end of the final block
  PNG_ERR_ADLER = 12,        // the Adler-32 trailer
  PNG_ERR_FILTER = 13        // a filter byte above 4 (set by the unfilter launch)
};

constexpr int PNG_WINDOW = 32768;
constexpr unsigned PNG_ADLER_MOD = 65521u;
constexpr int PNG_ROW_CAP = 24576;            // bytes of a row without its filter byte: the row kept in LDS between row groups
constexpr int PNG_DESC = 8;                   // ints per frame: W, H, colour type, bit depth, out channels, palette row, 0, 0

// What a frame's descriptor means, or ok == false.  rowbytes: bytes of a row after its filter byte; bpp: the filter's byte distance;
// expect: H (1 + rowbytes) filtered bytes; out_bytes: H W out channels.
struct PngPlan {
  bool ok;
  int W, H, ct, bd, och, prow, rowbytes, bpp;
  long long expect, out_bytes;
};

PNG_HD PngPlan png_plan(const int* d, int n_palettes, int max_rowbytes) {
  PngPlan p;
  p.W = d[0], p.H = d[1], p.ct = d[2], p.bd = d[3], p.och = d[4], p.prow = d[5];
  p.ok = false, p.rowbytes = 0, p.bpp = 1, p.expect = 0, p.out_bytes = 0;
  if (p.W < 1 || p.H < 1) return p;
  const bool depth = p.ct == 3 ? (p.bd == 1 || p.bd == 2 || p.bd == 4 || p.bd == 8) : ((p.ct == 0 || p.ct == 2) && p.bd == 8);
  if (!depth) return p;
  if (p.ct == 2 ? p.och != 3 : (p.och != 1 && p.och != 3)) return p;
  if (p.ct == 3 && p.och == 3 && (p.prow < 0 || p.prow >= n_palettes)) return p;
  const long long bits = (long long)p.W * (p.ct == 2 ? 24 : p.bd);
  const long long rb = (bits + 7) >> 3;
  if (rb > max_rowbytes || rb > PNG_ROW_CAP) return p;
  p.rowbytes = (int)rb;
  p.bpp = p.ct == 2 ? 3 : 1;
  p.expect = (long long)p.H * (1 + rb);
  p.out_bytes = (long long)p.H * p.W * p.och;
  p.ok = true;
  return p;
}

// ---- the bit reader: LSB first, at most 32 bits per request ----------------------------------------------------------------------------
struct PngBits {
  const uint8_t* in;
  long long pos, end;        // the next byte to load and the end of the frame's stream, both indices of `in`
  uint64_t buf;
  int cnt;
};

PNG_HD void png_refill(PngBits& b) {
  while (b.cnt <= 56 && b.pos < b.end) {      // (counted by bytes consumed)
    b.buf |= (uint64_t)b.in[b.pos++] << b.cnt;
    b.cnt += 8;
  }
}

// n <= 32 bits into *v; false: the input is exhausted
PNG_HD bool png_bits(PngBits& b, int n, unsigned* v) {
  if (b.cnt < n) png_refill(b);
  if (b.cnt < n) return false;
  *v = (unsigned)(b.buf & ((1ull << n) - 1));
  b.buf >>= n;
  b.cnt -= n;
  return true;
}

// ---- canonical Huffman tables by per-length counts -------------------------------------------------------------------------------------
struct PngTables {
  uint16_t lcount[16], lsym[288];             // literal / length code
  uint16_t dcount[16], dsym[32];              // distance code; the code-length code while a dynamic header is read
  uint16_t offs[16];
  uint8_t lens[320];                          // code lengths of a dynamic block: HLIT + HDIST <= 316
};

// count / sym of the n lengths `lens`.  Returns 0 for a complete code, > 0 for an incomplete and < 0 for an over-subscribed one;
// *coded: the symbols with a length.
PNG_HD int png_build(const uint8_t* lens, int n, uint16_t* count, uint16_t* sym, uint16_t* offs, int* coded) {
  for (int l = 0; l < 16; ++l) count[l] = 0;
  for (int i = 0; i < n; ++i) count[lens[i] & 15]++;
  *coded = n - count[0];
  int left = 1;
  for (int l = 1; l < 16; ++l) {
    left = (left << 1) - count[l];
    if (left < 0) return left;
  }
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
  for (int i = 0; i < n; ++i) {
    const int l = lens[i] & 15;
    if (l) sym[offs[l]++] = (uint16_t)i;      // offs[l] < coded <= n: inside sym
  }
  return left;
}

// zlib's rule for a code that is not complete: a single code of one bit, or (distances only: allow_none) no code at all
PNG_HD bool png_code_ok(int left, int coded, const uint16_t* count, bool allow_none) {
  if (left < 0) return false;
  if (left == 0) return true;
  return (coded == 1 && count[1] == 1) || (allow_none && coded == 0);
}

// One symbol, at most 15 steps.  -1: the bits are no code of the table; -2: the input is exhausted.
PNG_HD int png_decode(PngBits& b, const uint16_t* count, const uint16_t* sym) {
  if (b.cnt < 15) png_refill(b);
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; ++len) {
    code |= (int)((b.buf >> (len - 1)) & 1);
    const int c = count[len];
    if (code - c < first) {
      if (len > b.cnt) return -2;
      b.buf >>= len;
      b.cnt -= len;
      return sym[index + (code - first)];     // index + code - first < coded
    }
    index += c;
    first = (first + c) << 1;
    code <<= 1;
  }
  return b.cnt < 15 ? -2 : -1;
}

// ---- the output: `out` is written only, the last 32 KB are read back from `ring` --------------------------------------------------------
struct PngOut {
  uint8_t* out;              // the frame's region of the filtered buffer starts at out[0]
  uint8_t* ring;             // PNG_WINDOW bytes
  long long n, expect;       // bytes produced, bytes the frame has
  uint64_t sx, six;          // this lane's sum x and sum (i mod 65521) x over the bytes it stored
};

template <class L>
PNG_HD void png_put(PngOut& o, long long i, unsigned c) {     // i in [0, expect): checked by the callers
  o.ring[i & (PNG_WINDOW - 1)] = (uint8_t)c;
  o.out[i] = (uint8_t)c;
  o.sx += c;
  o.six += (uint64_t)(i % PNG_ADLER_MOD) * c;                 // < 2^24 per byte, < 2^31 bytes
}

template <class L>
PNG_HD int png_literal(PngOut& o, unsigned c) {
  if (o.n >= o.expect) return PNG_ERR_OVERFLOW;
  if (L::lane() == 0) png_put<L>(o, o.n, c);
  o.n += 1;
  return PNG_OK;
}

// len in [3, 258] bytes from `dist` back.  Lane j takes byte j from src[j % dist]: [n - dist, n) is complete before the copy starts
// and is not written by it (the ring places n + j on n + j - 32768 < n - dist + (j' % dist) for every j' >= j of a later round).
template <class L>
PNG_HD int png_match(PngOut& o, int len, int dist) {
  if (dist > o.n) return PNG_ERR_DISTANCE;
  if (o.n + len > o.expect) return PNG_ERR_OVERFLOW;
  L::sync();
  const long long from = o.n - dist;
  for (int j = L::lane(); j < len; j += L::N) {
    const int k = j < dist ? j : j % dist;
    png_put<L>(o, o.n + j, o.ring[(from + k) & (PNG_WINDOW - 1)]);
  }
  o.n += len;
  return PNG_OK;
}

// len bytes of a stored block from in[pos ...)
template <class L>
PNG_HD int png_stored(PngOut& o, PngBits& b, int len) {
  if (len > b.end - b.pos) return PNG_ERR_INPUT;
  if (o.n + len > o.expect) return PNG_ERR_OVERFLOW;
  for (int j = L::lane(); j < len; j += L::N) png_put<L>(o, o.n + j, b.in[b.pos + j]);
  b.pos += len;
  o.n += len;
  return PNG_OK;
}

PNG_HD void png_fixed_lengths(uint8_t* lens) {
  for (int i = 0; i < 288; ++i) lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  for (int i = 288; i < 320; ++i) lens[i] = 5;
}

// The header of a dynamic block into t->lens and the two tables
PNG_HD int png_dynamic_tables(PngBits& b, PngTables* t) {
  constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  unsigned v;
  if (!png_bits(b, 14, &v)) return PNG_ERR_INPUT;
  const int hlit = (int)(v & 31) + 257, hdist = (int)((v >> 5) & 31) + 1, hclen = (int)(v >> 10) + 4;
  if (hlit > 286 || hdist > 30) return PNG_ERR_CODE_LENGTHS;
  for (int i = 0; i < 19; ++i) t->lens[i] = 0;
  for (int i = 0; i < hclen; ++i) {
    if (!png_bits(b, 3, &v)) return PNG_ERR_INPUT;
    t->lens[order[i]] = (uint8_t)v;
  }
  int coded;
  if (png_build(t->lens, 19, t->dcount, t->dsym, t->offs, &coded) != 0) return PNG_ERR_CODE_LENGTHS;
  const int total = hlit + hdist;
  int idx = 0;
  while (idx < total) {                        // (every round consumes at least one bit and adds at least one length)
    const int s = png_decode(b, t->dcount, t->dsym);
    if (s < 0) return s == -2 ? PNG_ERR_INPUT : PNG_ERR_SYMBOL;
    if (s < 16) {
      t->lens[idx++] = (uint8_t)s;
      continue;
    }
    int rep, val = 0;
    if (s == 16) {
      if (idx == 0) return PNG_ERR_REPEAT;
      val = t->lens[idx - 1];
      if (!png_bits(b, 2, &v)) return PNG_ERR_INPUT;
      rep = 3 + (int)v;
    } else if (s == 17) {
      if (!png_bits(b, 3, &v)) return PNG_ERR_INPUT;
      rep = 3 + (int)v;
    } else {
      if (!png_bits(b, 7, &v)) return PNG_ERR_INPUT;
      rep = 11 + (int)v;
    }
    if (idx + rep > total) return PNG_ERR_REPEAT;
    for (int k = 0; k < rep; ++k) t->lens[idx++] = (uint8_t)val;
  }
  if (t->lens[256] == 0) return PNG_ERR_CODE_LENGTHS;
  int left = png_build(t->lens, hlit, t->lcount, t->lsym, t->offs, &coded);
  if (!png_code_ok(left, coded, t->lcount, false)) return PNG_ERR_CODE_LENGTHS;
  left = png_build(t->lens + hlit, hdist, t->dcount, t->dsym, t->offs, &coded);
  if (!png_code_ok(left, coded, t->dcount, true)) return PNG_ERR_CODE_LENGTHS;
  return PNG_OK;
}

// The symbols of one compressed block
template <class L>
PNG_HD int png_block(PngBits& b, const PngTables* t, PngOut& o) {
  for (;;) {                                   // (every round consumes at least one bit)
    int s = png_decode(b, t->lcount, t->lsym);
    if (s < 0) return s == -2 ? PNG_ERR_INPUT : PNG_ERR_SYMBOL;
    if (s < 256) {
      const int rc = png_literal<L>(o, (unsigned)s);
      if (rc) return rc;
      continue;
    }
    if (s == 256) return PNG_OK;
    if (s > 285) return PNG_ERR_SYMBOL;
    unsigned v = 0;
    int len;
    if (s < 265) {
      len = s - 254;
    } else if (s == 285) {
      len = 258;
    } else {
      const int e = (s - 261) >> 2;
      if (!png_bits(b, e, &v)) return PNG_ERR_INPUT;
      len = ((4 + ((s - 261) & 3)) << e) + 3 + (int)v;
    }
    const int d = png_decode(b, t->dcount, t->dsym);
    if (d < 0) return d == -2 ? PNG_ERR_INPUT : PNG_ERR_SYMBOL;
    if (d > 29) return PNG_ERR_SYMBOL;
    int dist;
    if (d < 4) {
      dist = d + 1;
    } else {
      const int e = (d >> 1) - 1;
      if (!png_bits(b, e, &v)) return PNG_ERR_INPUT;
      dist = ((2 + (d & 1)) << e) + 1 + (int)v;
    }
    const int rc = png_match<L>(o, len, dist);
    if (rc) return rc;
  }
}

// One zlib stream in[in_begin, in_end) into out[0, expect).  ring: PNG_WINDOW bytes, t: the tables, red: max(L::N, 4) words, all shared
// by the lanes.  *produced (NULL: not wanted): the bytes written (<= expect).  Returns the status.
template <class L>
PNG_HD int png_inflate(const uint8_t* in, long long in_begin, long long in_end, uint8_t* out, long long expect, uint8_t* ring, PngTables* t,
                       unsigned long long* red, long long* produced) {
  PngBits b = {in, in_begin, in_end, 0, 0};
  PngOut o = {out, ring, 0, expect, 0, 0};
  if (produced) *produced = 0;
  unsigned v;
  if (!png_bits(b, 16, &v)) return PNG_ERR_INPUT;
  const unsigned cmf = v & 255, flg = v >> 8;
  if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) return PNG_ERR_ZLIB_HEADER;
  int rc = PNG_OK;
  bool have_fixed = false;                     // the tables are the fixed code's already
  unsigned final_block = 0;
  while (!final_block) {                       // (every block consumes at least three bits)
    if (!png_bits(b, 3, &v)) {
      rc = PNG_ERR_INPUT;
      break;
    }
    final_block = v & 1;
    const unsigned type = v >> 1;
    if (type == 0) {
      b.buf >>= b.cnt & 7;
      b.cnt -= b.cnt & 7;
      if (!png_bits(b, 32, &v)) {
        rc = PNG_ERR_INPUT;
        break;
      }
      if ((v & 0xFFFF) != ((~v >> 16) & 0xFFFF)) {
        rc = PNG_ERR_STORED_LEN;
        break;
      }
      b.pos -= b.cnt >> 3;                     // whole bytes that the reader holds go back: pos stays in [in_begin, in_end]
      b.buf = 0, b.cnt = 0;
      rc = png_stored<L>(o, b, (int)(v & 0xFFFF));
    } else if (type == 3) {
      rc = PNG_ERR_BLOCK_TYPE;
    } else {
      L::sync();                               // the tables of the block before are no longer read
      if (L::lane() == 0) {
        if (type == 1) {
          if (!have_fixed) {
            int coded;
            png_fixed_lengths(t->lens);
            png_build(t->lens, 288, t->lcount, t->lsym, t->offs, &coded);
            png_build(t->lens + 288, 32, t->dcount, t->dsym, t->offs, &coded);
          }
          red[0] = PNG_OK;
        } else {
          PngBits b0 = b;
          red[0] = (unsigned long long)png_dynamic_tables(b0, t);
          red[1] = (unsigned long long)b0.pos, red[2] = b0.buf, red[3] = (unsigned long long)b0.cnt;
        }
      }
      L::sync();
      rc = (int)red[0];
      if (type == 2) b.pos = (long long)red[1], b.buf = red[2], b.cnt = (int)red[3];
      L::sync();                               // red is free again
      have_fixed = type == 1;
      if (rc == PNG_OK) rc = png_block<L>(b, t, o);
    }
    if (rc) break;
  }
  if (produced) *produced = o.n;
  if (rc) return rc;
  if (o.n != expect) return PNG_ERR_SHORT;
  b.buf >>= b.cnt & 7;
  b.cnt -= b.cnt & 7;
  if (!png_bits(b, 32, &v)) return PNG_ERR_INPUT;
  const unsigned want = ((v & 255) << 24) | ((v & 0xFF00) << 8) | ((v >> 8) & 0xFF00) | (v >> 24);
  // Adler-32 from the lanes' partial sums: a = 1 + sum x, b = n + n sum x - sum i x
  L::sync();
  red[L::lane()] = o.sx % PNG_ADLER_MOD;
  L::sync();
  uint64_t sx = 0, six = 0;
  for (int i = 0; i < L::N; ++i) sx += red[i];
  L::sync();
  red[L::lane()] = o.six % PNG_ADLER_MOD;
  L::sync();
  for (int i = 0; i < L::N; ++i) six += red[i];
  sx %= PNG_ADLER_MOD, six %= PNG_ADLER_MOD;
  const uint64_t nm = (uint64_t)(expect % PNG_ADLER_MOD);
  const unsigned a = (unsigned)((1 + sx) % PNG_ADLER_MOD);
  const unsigned bb = (unsigned)((nm + nm * sx + PNG_ADLER_MOD - six) % PNG_ADLER_MOD);
  return ((bb << 16) | a) == want ? PNG_OK : PNG_ERR_ADLER;
}

// ---- the row filters (PNG 1.2, section 6): recon = filt + pred(type, a, b, c) -------------------------------------------------------------
PNG_HD unsigned png_predict(int type, unsigned a, unsigned b, unsigned c) {
  if (type == 1) return a;
  if (type == 2) return b;
  if (type == 3) return (a + b) >> 1;          // on the 9-bit sum
  if (type == 4) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pc = p > (int)c ? p - (int)c : (int)c - p;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);   // ties: a, then b, then c
  }
  return 0;
}

}  // namespace univs
#endif  // UNIVS_PNG_INFLATE_CORE_H
