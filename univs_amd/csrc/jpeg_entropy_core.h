// The entropy decoder of the device JPEG reader (csrc/jpeg_decode.hip), as one host/device text: tools/jpeg_entropy_host.cpp compiles
// this very header for the host and runs the subsequence schedule lane by lane, plain and under the address and undefined-behaviour
// sanitizers (tests/test_jpeg_entropy_cpu.py), before a malformed byte reaches a GPU.  Same arrangement as png_inflate_core.h.
//
// The data is untrusted.  Every loop below is counted by bits consumed (a symbol is at least one bit) or by table entries; every load goes
// through JpegBits::byte, which answers 0 outside [0, nbytes) of the interval; every store is checked against the file's block buffer and
// against the blocks the interval still owes.
//
//   jpeg_byte_role     what a byte of the entropy-coded segment is, from itself and its two neighbours: kept, a stuffed 00 / fill FF /
//                      marker byte (dropped), the FF of an RSTn (cuts an interval), or the FF of any other marker (ends the data)
//   jpeg_build_table   a DHT (counts, values) pair -> JpegTable: an 8-bit first-level look-up and per-length limits for the longer codes
//   jpeg_decode_span   the decoder proper: from a state (bit position p, block of the MCU b, zig-zag index z) it decodes symbols until p
//                      passes `span_end`, counting completed blocks and per-component DC-difference sums; WRITE = false stores nothing
//                      and turns any rule break into a dead state (p = span_end, err set: normal for a speculative start), WRITE = true
//                      stores the coefficients de-zig-zagged with absolute DC and reports the break
//
// The overflow-synchronised schedule that calls it (phases 1 to 3) is in jpeg_decode.hip (jpeg_entropy_kernel) and, lane by lane, in the
// host tool; DESIGN.md has the argument why its fixpoint is the serial decode.
#ifndef UNIVS_JPEG_ENTROPY_CORE_H
#define UNIVS_JPEG_ENTROPY_CORE_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif

namespace univs {

// Per-file status: a set of bits, so that the workgroups of a file can OR theirs in.  0 = the file's pixels are Pillow's.
enum JpegStatus : int {
  JPEG_OK = 0,
  JPEG_ERR_DESC = 1,        // sizes, sampling, offsets or a region not admissible
  JPEG_ERR_TABLE = 2,       // a Huffman table with more than 256 values or an over-subscribed length
  JPEG_ERR_CODE = 4,        // bits that are no code
  JPEG_ERR_RUN = 8,         // a zero run past the end of the block
  JPEG_ERR_EXHAUSTED = 16,  // the interval's data ends before its blocks do
  JPEG_ERR_RESTART = 32,    // RSTn markers out of sequence, or not as many intervals as the restart interval and the frame give
  JPEG_ERR_CATEGORY = 64,   // a magnitude category above 11 (DC) / 10 (AC)
  JPEG_ERR_DC = 128,        // a DC value outside int16
  JPEG_ERR_RANGE = 256,     // not covered: |coef q| > 32767, a first-pass IDCT output outside int16, a second-pass value outside [-512, 511]
  JPEG_ERR_EOI = 512        // the data is not ended by an EOI marker
};

constexpr int JPEG_MAX_PER_MCU = 6;           // blocks of an MCU: at most 2 x 2 luma + Cb + Cr
constexpr int JPEG_TABLE_BYTES = 16 + 256;    // a Huffman table as uploaded: 16 counts, 256 values (padded with zeros)
constexpr int JPEG_WG = 1024;                // lanes of the workgroup that decodes an interval: subsequences per chunk
constexpr int JPEG_MAX_INTERVAL = 1 << 27;    // bytes of one interval: bit positions stay below 2^30

JPEG_HD int jpeg_zigzag(int z) {              // zig-zag index -> natural (row-major) index
  constexpr uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return nat[z & 63];
}

// ---- the pre-pass's rule ------------------------------------------------------------------------------------------------------------------------
enum JpegRole : int { JPEG_DROP = 0, JPEG_KEEP = 1, JPEG_RST = 2, JPEG_END = 4 };

// prev / next: the neighbouring bytes, 0 before the first and 0x100 after the last (a final FF ends the data, and is no EOI).
// An FF is always the first byte of a pair: FF 00 is the data byte FF, FF FF a fill byte, FF D0..D7 a restart marker, FF xx any other.
JPEG_HD int jpeg_byte_role(unsigned prev, unsigned cur, unsigned next) {
  if (cur == 0xFF) {
    if (next == 0x00) return JPEG_KEEP;
    if (next == 0xFF) return JPEG_DROP;
    return (next >= 0xD0 && next <= 0xD7) ? JPEG_RST : JPEG_END;
  }
  return prev == 0xFF ? JPEG_DROP : JPEG_KEEP;                      // the second byte of a pair
}

// ---- Huffman tables -----------------------------------------------------------------------------------------------------------------------------
struct JpegTable {
  uint16_t lut[256];   // by the next 8 bits: (length << 8) | value for a code of at most 8 bits, 0 else
  int32_t limit[17];   // by length l: the 16-bit look-ahead of a code of length <= l is below limit[l]
  int32_t base[17];    // by length l: index of a code's value = base[l] + (look-ahead >> (16 - l))
  uint8_t values[256];
};

// src: 16 counts and 256 values.  false: over-subscribed, or more than 256 values.
JPEG_HD bool jpeg_build_table(const uint8_t* src, JpegTable* t) {
  for (int i = 0; i < 256; ++i) t->lut[i] = 0, t->values[i] = src[16 + i];
  int code = 0, k = 0;
  t->limit[0] = 0, t->base[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = src[l - 1];
    if (k + n > 256 || code + n > (1 << l)) return false;
    t->base[l] = k - code;
    if (l <= 8) {
      for (int c = 0; c < n; ++c) {
        const int first = (code + c) << (8 - l);
        for (int j = 0; j < (1 << (8 - l)); ++j) t->lut[first + j] = (uint16_t)((l << 8) | src[16 + k + c]);
      }
    }
    code += n, k += n;
    t->limit[l] = code << (16 - l);
    code <<= 1;
  }
  return true;
}

// ---- the bit reader -----------------------------------------------------------------------------------------------------------------------------
struct JpegBits {
  const uint8_t* data;   // the interval's compacted bytes
  int nbytes;
  unsigned long long acc;  // the next bits, left-aligned
  int cnt;                 // valid bits in acc
  int next;                // the next byte to load
  JPEG_HD unsigned byte(int i) const { return (i >= 0 && i < nbytes) ? data[i] : 0u; }
  JPEG_HD void start(int p) {                                       // p >= 0
    acc = 0, cnt = 0, next = p >> 3;
    fill();
    acc <<= (p & 7), cnt -= (p & 7);
  }
  JPEG_HD void fill() {                                             // at most 8 loads; afterwards cnt > 56
    while (cnt <= 56) {
      acc |= (unsigned long long)byte(next) << (56 - cnt);
      ++next, cnt += 8;
    }
  }
  JPEG_HD unsigned peek16() const { return (unsigned)(acc >> 48); }
  JPEG_HD void drop(int n) { acc <<= n, cnt -= n; }                 // 0 <= n <= 16
  JPEG_HD unsigned take(int n) {                                    // 1 <= n <= 16
    const unsigned v = (unsigned)(acc >> (64 - n));
    drop(n);
    return v;
  }
};

// ---- the decoder --------------------------------------------------------------------------------------------------------------------------------
// p: bit position inside the interval; b: block inside the MCU; z: zig-zag index of the next coefficient (0: a DC symbol is next);
// n: blocks completed; dc: per component, the sum of the DC differences decoded; err: 0 or the JpegStatus bit of the rule broken
struct JpegState {
  int p, b, z, n;
  int dc[3];
  int err;
};

struct JpegScan {
  const uint8_t* data;     // the interval's compacted bytes
  int nbytes;
  int per, hv;             // blocks per MCU; luma blocks per MCU (h v); component of block b: b < hv ? 0 : 1 + b - hv
  const JpegTable* tab;    // [2 c]: DC table of component c, [2 c + 1]: its AC table
  const uint8_t* zz;       // [64] jpeg_zigzag
};

JPEG_HD int jpeg_component(const JpegScan& sc, int b) { return b < sc.hv ? 0 : 1 + b - sc.hv; }

// a[c] of three values without a runtime index (a runtime-indexed private array would leave the registers)
JPEG_HD int jpeg_pick3(const int* a, int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// The next symbol's (length, value) through `t`; length 0: no code
JPEG_HD int jpeg_symbol(const JpegTable& t, unsigned look, int* len) {
  const unsigned e = t.lut[look >> 8];
  if (e) {
    *len = (int)(e >> 8);
    return (int)(e & 255u);
  }
  for (int l = 9; l <= 16; ++l) {
    if ((int)look < t.limit[l]) {
      *len = l;
      return t.values[(t.base[l] + (int)(look >> (16 - l))) & 255];
    }
  }
  *len = 0;
  return 0;
}

// Decodes from `s` until s.p >= span_end (span_end <= 8 nbytes).  WRITE: coefficient (block n of this call, natural index i) goes to
// blocks[(block0 + n) 64 + i] while n < owed (the blocks the interval still expects from block0 on) and block0 + n < nblocks; with
// n == owed the call ends at once, the interval's blocks are complete.  pred: the DC predictors at s (WRITE only).
template <bool WRITE>
JPEG_HD void jpeg_decode_span(const JpegScan& sc, JpegState& s, int span_end, int16_t* blocks, long long nblocks, long long block0, int owed,
                              const int* pred) {
  JpegBits br{sc.data, sc.nbytes, 0, 0, 0};
  const int nbits = sc.nbytes * 8;
  if (s.p < 0 || s.b < 0 || s.b >= sc.per || s.z < 0 || s.z > 63) {  // (a state is data: it came through memory)
    s.err = JPEG_ERR_DESC, s.p = span_end;
    return;
  }
  if (s.p >= span_end) return;
  br.start(s.p);
  for (int guard = span_end - s.p; guard > 0; --guard) {            // a symbol is at least one bit
    if (s.p >= span_end) return;
    if (WRITE && s.n >= owed) return;
    br.fill();
    const int c = jpeg_component(sc, s.b);
    const JpegTable& t = sc.tab[2 * c + (s.z ? 1 : 0)];
    int len;
    const int sym = jpeg_symbol(t, br.peek16(), &len);
    int err = 0, run = 0, size = sym;
    if (len == 0) {                                                 // ((run < 15, 0) is the end of the block, as libjpeg reads it)
      err = JPEG_ERR_CODE;
    } else if (s.z == 0) {
      if (size > 11) err = JPEG_ERR_CATEGORY;
    } else {
      run = sym >> 4, size = sym & 15;
      if (size > 10) err = JPEG_ERR_CATEGORY;
      if (!err && size && s.z + run > 63) err = JPEG_ERR_RUN;
      if (!err && !size && run == 15 && s.z + 16 > 64) err = JPEG_ERR_RUN;
    }
    if (!err && s.p + len + size > nbits) err = JPEG_ERR_EXHAUSTED;
    if (err) {
      s.err = err;
      if (!WRITE) s.p = span_end;
      return;
    }
    br.drop(len);
    int v = 0;
    if (size) {
      v = (int)br.take(size);
      if (v < (1 << (size - 1))) v -= (1 << size) - 1;
    }
    s.p += len + size;
    const bool store = WRITE && s.n < owed && block0 + s.n >= 0 && block0 + s.n < nblocks;
    if (s.z == 0) {
      const int sum = (int)((unsigned)jpeg_pick3(s.dc, c) + (unsigned)v);
      s.dc[0] = c == 0 ? sum : s.dc[0], s.dc[1] = c == 1 ? sum : s.dc[1], s.dc[2] = c >= 2 ? sum : s.dc[2];
      if (WRITE) {
        const int dc = (int)((unsigned)jpeg_pick3(pred, c) + (unsigned)sum);
        if (dc < -32768 || dc > 32767) {
          s.err = JPEG_ERR_DC;
          return;
        }
        if (store) blocks[(block0 + s.n) * 64] = (int16_t)dc;
      }
      s.z = 1;
    } else if (size) {
      s.z += run;
      if (store) blocks[(block0 + s.n) * 64 + sc.zz[s.z]] = (int16_t)v;
      s.z += 1;
    } else {
      s.z = (sym >> 4) == 15 ? s.z + 16 : 64;                       // ZRL, or the end of the block
    }
    if (s.z >= 64) {
      s.z = 0, s.n += 1;
      s.b = s.b + 1 == sc.per ? 0 : s.b + 1;
    }
  }
}

}  // namespace univs
#endif  // UNIVS_JPEG_ENTROPY_CORE_H
