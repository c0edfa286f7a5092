// Baseline JPEG files encoded on the device (include/univs_jpegenc_hip.h): uint8 [N, H, W, 3] frames, optionally with a result
// overlaid on the fly, to the entropy-coded bytes of `PIL.Image.save(f, "JPEG", quality=q, subsampling=s)` bit for bit (the rule:
// data/jpeg_encode_rule.py and inference/overlay_rule.py).  The host writes the marker segments; five launches in two phases do the rest.
//
// Phase 1 (the coefficients and how many bits they take):
// jpegenc_blocks_kernel: 8 lanes per 8 x 8 block, 32 blocks per workgroup, in scan order.  Lane j fetches row j of the block: the pixel
// (blended with the overlay's colour, or the contour colour where a 4-neighbour inside the image has another id: no overlaid plane
// exists), colour conversion, edge replication and the chroma downsampling are all in the fetch.  It runs jfdctint.c's row pass, the
// block is transposed through LDS, lane j runs column j, quantises, and the block leaves through LDS in zig-zag order, 16 bytes a lane.
// A dummy block (beyond the component's blocks inside the last MCU column or row) is stored as zeros.
// jpegenc_sizes_kernel: a lane per block sums the lengths of its codes.  The DC difference is an index computation: the block before
// it of its component, and for a dummy the last real block before it in the MCU, whose DC it also stores, so `blocks` is complete.
// jpegenc_scan_kernel: a workgroup per frame, an exclusive scan of the sizes in steps of 1024 blocks: bit offsets and the frame's total.
//
// Phase 2 (the bytes; the host has sized the buffers from the totals):
// jpegenc_pack_kernel: a workgroup owns JPEGENC_PACK_BLOCKS consecutive blocks, hence a contiguous bit range; a lane per block ORs its
// codes into LDS words, the words leave byte-swapped (the stream is MSB first), whole words with plain stores and the two boundary
// words, which a neighbour shares, with atomic ORs into the zeroed buffer.  The lane of the last block pads the last byte with ones.
// jpegenc_stuff_kernel: a workgroup per frame, JPEGENC_STUFF_STEP bytes a step: flag the FF bytes, prefix sum, scatter with the 00s
// inserted; the inverse of jpeg_unstuff_kernel.  It writes the frame's length.
#include <stdint.h>

#include "jpeg_entropy_core.h"
#include "jpeg_huff_std.h"
#include "launchers.h"

namespace univs {

enum JpegEncStatus : int { JPEGENC_ERR_DC_CATEGORY = 1, JPEGENC_ERR_AC_CATEGORY = 2, JPEGENC_ERR_ROOM = 4 };

constexpr int JPEGENC_BLOCKS_THREADS = 256;                          // 32 blocks of 8 lanes
constexpr int JPEGENC_SIZES_THREADS = 256;
constexpr int JPEGENC_SCAN_THREADS = 1024;
constexpr int JPEGENC_PACK_BLOCKS = 128;                             // blocks, and lanes, of a pack workgroup
constexpr int JPEGENC_BLOCK_WORDS = 54;                              // 32-bit words that hold any block: 20 DC bits + 63 x 26 AC bits + 7 pad
constexpr int JPEGENC_STUFF_THREADS = 256;
constexpr int JPEGENC_STUFF_PER = 16;                                // bytes of a lane in a step
constexpr int JPEGENC_STUFF_STEP = JPEGENC_STUFF_THREADS * JPEGENC_STUFF_PER;

struct JpegEncGeom {
  int W, H, h, v;      // the frame; luma sampled h x v, chroma 1 x 1
  int mx, my, per;     // MCUs across and down, blocks of an MCU
  int wb, hb;          // luma blocks across and down (chroma: mx, my)
};
struct JpegEncQuant {
  unsigned short q[2][64];   // luminance, chrominance; natural order
};
struct JpegEncSource {
  const uint8_t* rgb;   // [N, H, W, 3]
  const void* ids;      // [N, H, W] uint8 or int32, or NULL: no overlay
  const uint8_t* lut;   // [K, 4]
  int ids_is_i32, K;
  int edge;             // 0xRRGGBB, or -1: no contour
};

__host__ __device__ inline JpegEncGeom jpegenc_geom(int W, int H, int h, int v) {
  JpegEncGeom g;
  g.W = W, g.H = H, g.h = h, g.v = v;
  g.mx = (W + 8 * h - 1) / (8 * h), g.my = (H + 8 * v - 1) / (8 * v), g.per = h * v + 2;
  g.wb = (W + 7) / 8, g.hb = (H + 7) / 8;
  return g;
}

// Block k of MCU `mcu`: its component and its place among the component's blocks; true where it is a dummy
__device__ __forceinline__ bool jpegenc_locate(const JpegEncGeom& g, int mcu, int k, int* c, int* bx, int* by) {
  const int my_ = mcu / g.mx, mx_ = mcu - my_ * g.mx, nl = g.h * g.v;
  if (k >= nl) {
    *c = 1 + k - nl, *bx = mx_, *by = my_;
    return false;
  }
  const int r = k / g.h;
  *c = 0, *bx = mx_ * g.h + (k - r * g.h), *by = my_ * g.v + r;
  return *bx >= g.wb || *by >= g.hb;
}

// The block whose DC block b codes: b itself, or for a dummy the last real block before it in its MCU (block 0 of an MCU is real)
__device__ __forceinline__ int jpegenc_real(const JpegEncGeom& g, int b) {
  const int mcu = b / g.per;
  int k = b - mcu * g.per, c, bx, by;
  while (k > 0 && jpegenc_locate(g, mcu, k, &c, &bx, &by)) --k;
  return mcu * g.per + k;
}

// The block before b of its component in scan order; -1 for the component's first
__device__ __forceinline__ int jpegenc_before(const JpegEncGeom& g, int b) {
  const int mcu = b / g.per, k = b - mcu * g.per, nl = g.h * g.v;
  if (k >= nl) return mcu > 0 ? b - g.per : -1;
  if (k > 0) return b - 1;
  return mcu > 0 ? (mcu - 1) * g.per + nl - 1 : -1;
}

__device__ __forceinline__ int jpegenc_id(const JpegEncSource& s, long long at) {
  const int id = s.ids_is_i32 ? static_cast<const int*>(s.ids)[at] : (int)static_cast<const uint8_t*>(s.ids)[at];
  return min(max(id, 0), s.K - 1);
}

// The pixel (x, y) of frame f, inside the image, as it is encoded: the frame's, or the overlay's (inference/overlay_rule.py)
__device__ __forceinline__ void jpegenc_pixel(const JpegEncSource& s, const JpegEncGeom& g, int f, int x, int y, int* r, int* gr, int* b) {
  const long long at = ((long long)f * g.H + y) * g.W + x;
  const uint8_t* p = s.rgb + 3 * at;
  *r = p[0], *gr = p[1], *b = p[2];
  if (!s.ids) return;
  const int k = jpegenc_id(s, at);
  const uint8_t* l = s.lut + 4 * k;
  const int a = l[3];
  if (a == 0) return;
  if (s.edge >= 0) {
    const bool differs = (x > 0 && jpegenc_id(s, at - 1) != k) || (x + 1 < g.W && jpegenc_id(s, at + 1) != k) ||
                         (y > 0 && jpegenc_id(s, at - g.W) != k) || (y + 1 < g.H && jpegenc_id(s, at + g.W) != k);
    if (differs) {
      *r = (s.edge >> 16) & 255, *gr = (s.edge >> 8) & 255, *b = s.edge & 255;
      return;
    }
  }
  *r = (*r * (255 - a) + l[0] * a + 127) / 255;
  *gr = (*gr * (255 - a) + l[1] * a + 127) / 255;
  *b = (*b * (255 - a) + l[2] * a + 127) / 255;
}

// Component c of the pixel (x, y), both clamped into the image: the replication of the last column and row at full resolution
__device__ __forceinline__ int jpegenc_ycc(const JpegEncSource& s, const JpegEncGeom& g, int f, int c, int x, int y) {
  int r, gr, b;
  jpegenc_pixel(s, g, f, min(x, g.W - 1), min(y, g.H - 1), &r, &gr, &b);
  if (c == 0) return (19595 * r + 38470 * gr + 7471 * b + 32768) >> 16;
  if (c == 1) return (-11059 * r - 21709 * gr + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * gr - 5329 * b + (128 << 16) + 32767) >> 16;
}

// Sample (x, y) of component c's plane, padded to whole blocks
__device__ __forceinline__ int jpegenc_sample(const JpegEncSource& s, const JpegEncGeom& g, int f, int c, int x, int y) {
  if (c == 0 || (g.h == 1 && g.v == 1)) return jpegenc_ycc(s, g, f, c, x, y);
  if (g.v == 1) return (jpegenc_ycc(s, g, f, c, 2 * x, y) + jpegenc_ycc(s, g, f, c, 2 * x + 1, y) + (x & 1)) >> 1;
  y = min(y, (g.H + 1) / 2 - 1);                                     // below the image the last *downsampled* row repeats
  return (jpegenc_ycc(s, g, f, c, 2 * x, 2 * y) + jpegenc_ycc(s, g, f, c, 2 * x + 1, 2 * y) + jpegenc_ycc(s, g, f, c, 2 * x, 2 * y + 1) +
          jpegenc_ycc(s, g, f, c, 2 * x + 1, 2 * y + 1) + 1 + (x & 1)) >> 2;
}

// Whether frame f's region of the stream buffers, raw_off[f] .. raw_off[f + 1], is admissible and holds its `nbytes`, rounded up to words
__device__ __forceinline__ bool jpegenc_room(const long long* __restrict__ raw_off, int f, long long raw_total, long long nbytes) {
  const long long a = raw_off[f], b = raw_off[f + 1];
  return a >= 0 && !(a & 3) && b <= raw_total && b - a >= ((nbytes + 3) & ~3LL);
}

// jfdctint.c's one-dimensional pass, in place; the true value of every sum fits 32 bits
template <bool FIRST>
__device__ __forceinline__ void jpegenc_fdct_pass(int* d) {
  constexpr int n = FIRST ? 11 : 15, half = 1 << (n - 1);
  const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
  const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (FIRST) {
    d[0] = (tmp10 + tmp11) * 4;
    d[4] = (tmp10 - tmp11) * 4;
  } else {
    d[0] = (tmp10 + tmp11 + 2) >> 2;
    d[4] = (tmp10 - tmp11 + 2) >> 2;
  }
  int z1 = (tmp12 + tmp13) * 4433;
  d[2] = (z1 + tmp13 * 6270 + half) >> n;
  d[6] = (z1 - tmp12 * 15137 + half) >> n;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * 9633;
  const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  d[7] = (t4 + z1 + z3 + half) >> n;
  d[5] = (t5 + z2 + z4 + half) >> n;
  d[3] = (t6 + z2 + z3 + half) >> n;
  d[1] = (t7 + z1 + z4 + half) >> n;
}

__global__ __launch_bounds__(JPEGENC_BLOCKS_THREADS) void jpegenc_blocks_kernel(JpegEncSource s, JpegEncGeom g, JpegEncQuant quant, int nblocks,
                                                                                int16_t* __restrict__ blocks) {
  constexpr int G = JPEGENC_BLOCKS_THREADS / 8;
  __shared__ int tile[G][8][9];
  __shared__ int16_t nat[G][64];
  __shared__ unsigned short sq[2][64];
  const int t = threadIdx.x, grp = t >> 3, j = t & 7, f = blockIdx.y;
  const int b = blockIdx.x * G + grp;
  if (t < 128) sq[t >> 6][t & 63] = quant.q[t >> 6][t & 63];
  int c = 0, bx = 0, by = 0;
  const bool valid = b < nblocks;
  const bool dummy = valid ? jpegenc_locate(g, b / g.per, b % g.per, &c, &bx, &by) : true;
  int d[8];
  if (!dummy) {
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = jpegenc_sample(s, g, f, c, bx * 8 + i, by * 8 + j) - 128;
    jpegenc_fdct_pass<true>(d);
#pragma unroll
    for (int i = 0; i < 8; ++i) tile[grp][j][i] = d[i];
  }
  __syncthreads();
  if (!dummy) {
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = tile[grp][i][j];
    jpegenc_fdct_pass<false>(d);
    const int tq = c == 0 ? 0 : 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int q8 = (int)sq[tq][i * 8 + j] << 3, x = d[i];
      const int m = ((x < 0 ? -x : x) + (q8 >> 1)) / q8;
      nat[grp][i * 8 + j] = (int16_t)(x < 0 ? -m : m);
    }
  }
  __syncthreads();
  if (!valid) return;
  alignas(16) int16_t o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = dummy ? (int16_t)0 : nat[grp][jpeg_zigzag(8 * j + i)];
  *reinterpret_cast<int4*>(blocks + ((long long)f * nblocks + b) * 64 + 8 * j) = *reinterpret_cast<const int4*>(o);
}

__device__ __forceinline__ int jpegenc_category(int x) { return 32 - __clz(x < 0 ? -x : x); }   // (__clz(0) is 32)

// A block's symbols in order: emit(code, length) per DC and AC symbol with its magnitude bits appended, ZRL and EOB included.
// Returns the status bits.
template <class Emit>
__device__ __forceinline__ int jpegenc_symbols(const int16_t* __restrict__ blk, int dc_diff, int table, Emit&& emit) {
  int st = 0, s = jpegenc_category(dc_diff);
  if (s > 11) st |= JPEGENC_ERR_DC_CATEGORY, s = 11;
  unsigned e = JPEG_STD_DC[table][s];
  emit(((e & 0xFFFFu) << s) | ((unsigned)(dc_diff < 0 ? dc_diff - 1 : dc_diff) & ((1u << s) - 1u)), (int)(e >> 16) + s);
  int run = 0;
  for (int w = 0; w < 8; ++w) {
    alignas(16) int16_t v[8];
    *reinterpret_cast<int4*>(v) = *reinterpret_cast<const int4*>(blk + 8 * w);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (w == 0 && i == 0) continue;
      const int x = v[i];
      if (x == 0) {
        ++run;
        continue;
      }
      while (run > 15) {
        e = JPEG_STD_AC[table][0xF0];
        emit(e & 0xFFFFu, (int)(e >> 16));
        run -= 16;
      }
      s = jpegenc_category(x);
      if (s > 10) st |= JPEGENC_ERR_AC_CATEGORY, s = 10;
      e = JPEG_STD_AC[table][16 * run + s];
      emit(((e & 0xFFFFu) << s) | ((unsigned)(x < 0 ? x - 1 : x) & ((1u << s) - 1u)), (int)(e >> 16) + s);
      run = 0;
    }
  }
  if (run) {
    e = JPEG_STD_AC[table][0];
    emit(e & 0xFFFFu, (int)(e >> 16));
  }
  return st;
}

// The difference block b codes as its DC, from the stored DCs of real blocks only
__device__ __forceinline__ int jpegenc_dc_diff(const JpegEncGeom& g, const int16_t* __restrict__ frame_blocks, int b, int* dc) {
  const int before = jpegenc_before(g, b);
  *dc = frame_blocks[(long long)jpegenc_real(g, b) * 64];
  return *dc - (before < 0 ? 0 : (int)frame_blocks[(long long)jpegenc_real(g, before) * 64]);
}

__global__ __launch_bounds__(JPEGENC_SIZES_THREADS) void jpegenc_sizes_kernel(JpegEncGeom g, int nblocks, int16_t* __restrict__ blocks,
                                                                              unsigned* __restrict__ sizes, int* __restrict__ status) {
  const int b = blockIdx.x * JPEGENC_SIZES_THREADS + threadIdx.x, f = blockIdx.y;
  if (b >= nblocks) return;
  int16_t* frame_blocks = blocks + (long long)f * nblocks * 64;
  int dc;
  const int diff = jpegenc_dc_diff(g, frame_blocks, b, &dc);
  unsigned bits = 0;
  const int st = jpegenc_symbols(frame_blocks + (long long)b * 64, diff, b % g.per < g.h * g.v ? 0 : 1, [&](unsigned, int len) { bits += len; });
  if (jpegenc_real(g, b) != b) frame_blocks[(long long)b * 64] = (int16_t)dc;   // (no lane reads a dummy's DC: jpegenc_dc_diff)
  sizes[(long long)f * nblocks + b] = bits;
  if (st) atomicOr(status + f, st);
}

__global__ __launch_bounds__(JPEGENC_SCAN_THREADS) void jpegenc_scan_kernel(int nblocks, const unsigned* __restrict__ sizes,
                                                                            long long* __restrict__ bit_off, long long* __restrict__ totals) {
  __shared__ unsigned wave_tot[JPEGENC_SCAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, f = blockIdx.x;
  long long carry = 0;
  for (int base = 0; base < nblocks; base += JPEGENC_SCAN_THREADS) {
    const int b = base + t;
    const unsigned v = b < nblocks ? sizes[(long long)f * nblocks + b] : 0u;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = (unsigned)__shfl_up((int)inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int k = 0; k < JPEGENC_SCAN_THREADS / 64; ++k) {
      const unsigned x = wave_tot[k];
      before += k < w ? x : 0u;
      all += x;
    }
    __syncthreads();
    if (b < nblocks) bit_off[(long long)f * nblocks + b] = carry + before + inc - v;
    carry += all;
  }
  if (t == 0) totals[f] = carry;
}

__global__ __launch_bounds__(JPEGENC_PACK_BLOCKS) void jpegenc_pack_kernel(JpegEncGeom g, int nblocks, const int16_t* __restrict__ blocks,
                                                                           const long long* __restrict__ bit_off,
                                                                           const long long* __restrict__ totals,
                                                                           const long long* __restrict__ raw_off, long long raw_total,
                                                                           unsigned* __restrict__ raw, int* __restrict__ status) {
  __shared__ unsigned words[JPEGENC_PACK_BLOCKS * JPEGENC_BLOCK_WORDS + 2];
  const int t = threadIdx.x, f = blockIdx.y;
  if (!jpegenc_room(raw_off, f, raw_total, (totals[f] + 7) >> 3)) {  // (the whole workgroup: nothing of the frame is written)
    if (t == 0) atomicOr(status + f, (int)JPEGENC_ERR_ROOM);
    return;
  }
  const int first = blockIdx.x * JPEGENC_PACK_BLOCKS, last = min(first + JPEGENC_PACK_BLOCKS, nblocks);
  const long long* off = bit_off + (long long)f * nblocks;
  const long long total = totals[f];
  const long long g0 = off[first], g1 = last == nblocks ? ((total + 7) & ~7LL) : off[last];
  const long long w0 = g0 >> 5;
  const int nwords = (int)(((g1 + 31) >> 5) - w0);                   // at most PACK_BLOCKS BLOCK_WORDS + 1: a block's bits, pad included, fit BLOCK_WORDS
  for (int i = t; i < nwords; i += JPEGENC_PACK_BLOCKS) words[i] = 0u;
  __syncthreads();
  const int b = first + t;
  if (b < last) {
    const int16_t* frame_blocks = blocks + (long long)f * nblocks * 64;
    int dc;
    const int diff = jpegenc_dc_diff(g, frame_blocks, b, &dc);
    int p = (int)(off[b] - (w0 << 5));
    auto put = [&](unsigned code, int len) {                         // len <= 27: at most two words
      const int w = p >> 5, o = p & 31;
      const unsigned long long x = (unsigned long long)code << (64 - o - len);
      atomicOr(&words[w], (unsigned)(x >> 32));
      if ((unsigned)x) atomicOr(&words[w + 1], (unsigned)x);
      p += len;
    };
    jpegenc_symbols(frame_blocks + (long long)b * 64, diff, b % g.per < g.h * g.v ? 0 : 1, put);
    if (b == nblocks - 1) {
      const int pad = (int)(-total & 7);
      if (pad) put((1u << pad) - 1u, pad);
    }
  }
  __syncthreads();
  unsigned* dst = raw + (raw_off[f] >> 2) + w0;
  for (int i = t; i < nwords; i += JPEGENC_PACK_BLOCKS) {
    const unsigned x = __builtin_bswap32(words[i]);
    if (i == 0 || i == nwords - 1)
      atomicOr(dst + i, x);
    else
      dst[i] = x;
  }
}

__global__ __launch_bounds__(JPEGENC_STUFF_THREADS) void jpegenc_stuff_kernel(const long long* __restrict__ totals,
                                                                              const long long* __restrict__ raw_off, long long raw_total,
                                                                              const uint8_t* __restrict__ raw, uint8_t* __restrict__ out,
                                                                              long long* __restrict__ out_len) {
  __shared__ unsigned wave_tot[JPEGENC_STUFF_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, f = blockIdx.x;
  const long long nbytes = (totals[f] + 7) >> 3;
  if (!jpegenc_room(raw_off, f, raw_total, nbytes)) {                // (the pack launch has set the status)
    if (t == 0) out_len[f] = 0;
    return;
  }
  const uint8_t* src = raw + raw_off[f];
  uint8_t* dst = out + 2 * raw_off[f];
  long long carry = 0;                                               // FF bytes before this step
  for (long long base = 0; base < nbytes; base += JPEGENC_STUFF_STEP) {
    const long long at = base + (long long)t * JPEGENC_STUFF_PER;
    const int n = (int)max(0LL, min((long long)JPEGENC_STUFF_PER, nbytes - at));
    uint8_t v[JPEGENC_STUFF_PER];
    unsigned ff = 0;
#pragma unroll
    for (int i = 0; i < JPEGENC_STUFF_PER; ++i) {
      v[i] = i < n ? src[at + i] : (uint8_t)0;
      ff += v[i] == 0xFF;
    }
    unsigned inc = ff;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned o = (unsigned)__shfl_up((int)inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
    for (int k = 0; k < JPEGENC_STUFF_THREADS / 64; ++k) {
      const unsigned x = wave_tot[k];
      before += k < w ? x : 0u;
      all += x;
    }
    __syncthreads();
    long long o = at + carry + before + inc - ff;
#pragma unroll
    for (int i = 0; i < JPEGENC_STUFF_PER; ++i) {
      if (i < n) {
        dst[o++] = v[i];
        if (v[i] == 0xFF) dst[o++] = 0;
      }
    }
    carry += all;
  }
  if (t == 0) out_len[f] = nbytes + carry;
}

// ITU T.81 Annex K.1 / K.2 scaled as libjpeg's jpeg_set_quality does
static JpegEncQuant jpegenc_quant(int quality) {
  static const unsigned char base[2][64] = {
      {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
      {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  JpegEncQuant q;
  for (int tq = 0; tq < 2; ++tq)
    for (int i = 0; i < 64; ++i) {
      const int x = (base[tq][i] * scale + 50) / 100;
      q.q[tq][i] = (unsigned short)(x < 1 ? 1 : x > 255 ? 255 : x);
    }
  return q;
}

int jpeg_encode(const unsigned char* rgb, const void* ids, int ids_is_i32, const unsigned char* lut, int K, int edge, int N, int H, int W, int h,
                int v, int quality, int phases, short* blocks, unsigned* sizes, long long* bit_off, long long* totals, const long long* raw_off,
                long long raw_total, unsigned char* raw, unsigned char* out, long long* out_len, int* status, hipStream_t st) {
  const bool sampling = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
  if (!sampling || W < 1 || H < 1 || W > 16384 || H > 16384 || quality < 1 || quality > 100 || 3LL * N * H * W >= (1LL << 31) ||
      raw_total >= (1LL << 40) || (reinterpret_cast<uintptr_t>(blocks) & 15) || (reinterpret_cast<uintptr_t>(raw) & 3))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  const JpegEncGeom g = jpegenc_geom(W, H, h, v);
  const int nblocks = g.mx * g.my * g.per;                           // at most 2048 x 2048 x 3 (4:4:4)
  if (phases & 1) {
    if (hipMemsetAsync(status, 0, sizeof(int) * N, st) != hipSuccess) {
      (void)hipGetLastError();
      set_error("jpeg_encode: clearing the status failed");
      return UNIVS_ERR_LAUNCH;
    }
    const JpegEncSource s = {rgb, ids, lut, ids_is_i32, K, ids ? edge : -1};
    constexpr int per_wg = JPEGENC_BLOCKS_THREADS / 8;
    hipLaunchKernelGGL(jpegenc_blocks_kernel, dim3((unsigned)((nblocks + per_wg - 1) / per_wg), (unsigned)N), dim3(JPEGENC_BLOCKS_THREADS), 0, st, s,
                       g, jpegenc_quant(quality), nblocks, blocks);
    hipLaunchKernelGGL(jpegenc_sizes_kernel, dim3((unsigned)((nblocks + JPEGENC_SIZES_THREADS - 1) / JPEGENC_SIZES_THREADS), (unsigned)N),
                       dim3(JPEGENC_SIZES_THREADS), 0, st, g, nblocks, blocks, sizes, status);
    hipLaunchKernelGGL(jpegenc_scan_kernel, dim3((unsigned)N), dim3(JPEGENC_SCAN_THREADS), 0, st, nblocks, sizes, bit_off, totals);
  }
  if (phases & 2) {
    if (hipMemsetAsync(raw, 0, (size_t)raw_total, st) != hipSuccess) {
      (void)hipGetLastError();
      set_error("jpeg_encode: clearing the stream buffer failed");
      return UNIVS_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jpegenc_pack_kernel, dim3((unsigned)((nblocks + JPEGENC_PACK_BLOCKS - 1) / JPEGENC_PACK_BLOCKS), (unsigned)N),
                       dim3(JPEGENC_PACK_BLOCKS), 0, st, g, nblocks, blocks, bit_off, totals, raw_off, raw_total,
                       reinterpret_cast<unsigned*>(raw), status);
    hipLaunchKernelGGL(jpegenc_stuff_kernel, dim3((unsigned)N), dim3(JPEGENC_STUFF_THREADS), 0, st, totals, raw_off, raw_total, raw, out,
                       out_len);
  }
  return check_launch("jpeg_encode");
}

}  // namespace univs
