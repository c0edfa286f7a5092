// Baseline JPEG frames decoded on the device (include/univs_jpeg_hip.h): the files of one video that share size and sampling, from their
// entropy-coded bytes to uint8 [N, H, W, 3], np.asarray(PIL.Image.open(f).convert("RGB")) bit for bit (the rule: data/jpeg_rule.py).  The host
// parses the marker segments and uploads tables and bytes; four launches do the rest.
//
// jpeg_unstuff_kernel, one workgroup per file.  A byte's role (kept, stuffed 00 / fill / marker byte, RSTn, end of data) depends on itself
// and its two neighbours only (jpeg_byte_role), so the kept bytes are compacted by a flag + prefix sum, 4096 bytes per step, and the RSTn
// markers cut the data into intervals whose starts go to `ivl`.  The marker numbers, the number of intervals and the EOI are checked here.
//
// jpeg_entropy_kernel, one workgroup of JPEG_WG lanes per interval: the overflow-synchronised parallel Huffman decode.  The interval is cut
// into subsequences of subseq_bits, a lane each, JPEG_WG per chunk.  Phase 1: every lane decodes its subsequence from the default state
// (block 0 of an MCU, a DC symbol next) without storing and records the state it leaves with.  Phase 2: lane i + 1 decodes again from
// lane i's exit wherever that differs from what it started with, until no start changes: a counted loop of at most (lanes - 1) rounds;
// after round r the first r + 1 lanes are the serial decode's, because lane 0 starts from the chunk's true state (the chunk before is
// complete) and a lane's exit is a function of its start alone.  Phase 3: exclusive scans of the block counts and DC-difference sums give
// every lane its block offset and predictors, and the write pass stores the coefficients, de-zig-zagged, with absolute DC.  The serial text
// (tables, bit reader, symbol decode, every bounds decision) is jpeg_entropy_core.h, which tools/jpeg_entropy_host.cpp runs on the host.
//
// jpeg_idct_kernel: 8 lanes per block, lane j runs column j, the block is transposed through LDS, lane j runs row j and stores 8 bytes of
// the component's plane (padded to whole MCUs).  jidctint.c's arithmetic in 32 bits: every product and sum is taken modulo 2^32 and the
// true value of every descaled sum fits (|input| <= 32767 times the absolute row sum of the scaled basis, 61 200, is below 2^31).  The
// three range conditions under which libjpeg-turbo's SIMD and C code can part are OR-ed into the file's status.
//
// jpeg_colour_kernel: a lane per output pixel reads luma and the chroma samples its triangle filter needs from the planes (no upsampled
// plane exists), converts, and the workgroup's 768 bytes leave through LDS as 192 aligned dwords.
#include <stdint.h>

#include "jpeg_entropy_core.h"
#include "launchers.h"

namespace univs {

// Exclusive prefix sum over the workgroup (blockDim.x a multiple of 64, at most 1024); sums modulo 2^32.  Two barriers.
__device__ __forceinline__ unsigned jpeg_scan(unsigned v, unsigned* wave_tot, unsigned* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned o = (unsigned)__shfl_up((int)inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_tot[w] = inc;
  __syncthreads();
  unsigned before = 0, all = 0;
  for (int k = 0; k < nw; ++k) {
    const unsigned x = wave_tot[k];
    before += k < w ? x : 0u;
    all += x;
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

// The file's region of the source / compacted buffer and its restart interval in MCUs; false where not admissible
__device__ __forceinline__ bool jpeg_file(int f, const long long* __restrict__ src_off, const int* __restrict__ ri, long long src_total, int mcus,
                                          int max_intervals, long long* s0, int* len, int* r, int* n_int) {
  const long long a = src_off[f], b = src_off[f + 1];
  if (a < 0 || b < a || b > src_total || b - a >= (1LL << 31)) return false;
  int q = ri[f];
  if (q <= 0 || q > mcus) q = mcus;
  *s0 = a, *len = (int)(b - a), *r = q, *n_int = (mcus + q - 1) / q;
  return *n_int <= max_intervals;
}

constexpr int JPEG_UNSTUFF_THREADS = 256;
constexpr int JPEG_UNSTUFF_PER = 16;

__global__ __launch_bounds__(JPEG_UNSTUFF_THREADS) void jpeg_unstuff_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ src_off,
                                                                            const int* __restrict__ ri, long long src_total, int mcus,
                                                                            int max_intervals, uint8_t* __restrict__ comp, int* __restrict__ ivl,
                                                                            int* __restrict__ status) {
  __shared__ unsigned wave_tot[JPEG_UNSTUFF_THREADS / 64];
  __shared__ int end_at, errs;
  const int f = blockIdx.x, t = threadIdx.x;
  long long s0;
  int len, r, n_int;
  if (!jpeg_file(f, src_off, ri, src_total, mcus, max_intervals, &s0, &len, &r, &n_int)) {
    if (t == 0) atomicOr(&status[f], JPEG_ERR_DESC);
    return;
  }
  const uint8_t* __restrict__ in = src + s0;
  uint8_t* __restrict__ out = comp + s0;                             // (the kept bytes are never more than the bytes read)
  int* __restrict__ iv = ivl + (long long)f * (max_intervals + 1);
  if (t == 0) end_at = len, errs = 0;
  __syncthreads();
  int kept = 0, nrst = 0;
  bool ended = false;
  constexpr int STEP = JPEG_UNSTUFF_THREADS * JPEG_UNSTUFF_PER;
  for (int base = 0; base < len; base += STEP) {
    const int i0 = base + t * JPEG_UNSTUFF_PER;
    unsigned b[JPEG_UNSTUFF_PER + 2];
#pragma unroll
    for (int j = 0; j < JPEG_UNSTUFF_PER + 2; ++j) {
      const int i = i0 + j - 1;
      b[j] = i < 0 ? 0u : (i < len ? in[i] : 0x100u);
    }
    int role[JPEG_UNSTUFF_PER];
    int first_end = len;
#pragma unroll
    for (int j = JPEG_UNSTUFF_PER - 1; j >= 0; --j) {
      role[j] = i0 + j < len ? jpeg_byte_role(b[j], b[j + 1], b[j + 2]) : JPEG_DROP;
      if (role[j] == JPEG_END) first_end = i0 + j;
    }
    if (first_end < len) atomicMin(&end_at, first_end);
    __syncthreads();
    const int end = end_at;                                          // the first byte that ends the data, len while there is none
    unsigned mine = 0;                                               // kept bytes in the low half, restart markers in the high half
#pragma unroll
    for (int j = 0; j < JPEG_UNSTUFF_PER; ++j) {
      if (i0 + j >= end) role[j] = JPEG_DROP;
      mine += role[j] == JPEG_KEEP ? 1u : (role[j] == JPEG_RST ? 0x10000u : 0u);
    }
    unsigned total;
    const unsigned before = jpeg_scan(mine, wave_tot, &total);
    int pos = kept + (int)(before & 0xFFFFu), idx = nrst + (int)(before >> 16), err = 0;
#pragma unroll
    for (int j = 0; j < JPEG_UNSTUFF_PER; ++j) {
      if (role[j] == JPEG_KEEP) {
        if (pos < len) out[pos] = (uint8_t)b[j + 1];
        ++pos;
      } else if (role[j] == JPEG_RST) {
        if ((int)b[j + 2] - 0xD0 != (idx & 7)) err |= JPEG_ERR_RESTART;
        if (idx + 1 < n_int) iv[idx + 1] = pos;
        else err |= JPEG_ERR_RESTART;
        ++idx;
      }
    }
    if (err) atomicOr(&errs, err);
    kept += (int)(total & 0xFFFFu), nrst += (int)(total >> 16);
    if (end < len) {                                                 // (uniform)
      ended = true;
      if (t == 0 && !(end + 1 < len && in[end + 1] == 0xD9)) atomicOr(&errs, JPEG_ERR_EOI);
      break;
    }
  }
  __syncthreads();
  if (t == 0) {
    int err = errs;
    if (!ended) err |= JPEG_ERR_EOI;
    if (nrst + 1 != n_int) err |= JPEG_ERR_RESTART;
    iv[0] = 0;
    if (nrst + 1 == n_int) iv[n_int] = kept;
    if (err) atomicOr(&status[f], err);
  }
}

__device__ __forceinline__ JpegState jpeg_fresh(int p, int bz) { return JpegState{p, bz >> 8, bz & 255, 0, {0, 0, 0}, 0}; }

__global__ __launch_bounds__(JPEG_WG) void jpeg_entropy_kernel(const uint8_t* __restrict__ comp, const long long* __restrict__ src_off,
                                                               const int* __restrict__ ri, const uint8_t* __restrict__ huff,
                                                               const int* __restrict__ ivl, long long src_total, int mcus, int per, int hv, int ntab,
                                                               int subseq_bits, int max_intervals, int16_t* __restrict__ blocks,
                                                               int* __restrict__ status, int* __restrict__ rounds) {
  __shared__ JpegTable tab[JPEG_MAX_PER_MCU];
  __shared__ uint8_t zz[64];
  __shared__ int ex_p[JPEG_WG], ex_bz[JPEG_WG];
  __shared__ unsigned wave_tot[JPEG_WG / 64];
  const int f = blockIdx.y, k = blockIdx.x, t = threadIdx.x;
  // the pre-pass's answer, read once for the workgroup: the workgroups of the file's other intervals may be OR-ing theirs in by now
  if (__syncthreads_or(t == 0 && status[f] != JPEG_OK)) return;
  long long s0;
  int len, r, n_int;
  if (!jpeg_file(f, src_off, ri, src_total, mcus, max_intervals, &s0, &len, &r, &n_int)) return;   // (the pre-pass has said so)
  if (k >= n_int) return;
  const int* __restrict__ iv = ivl + (long long)f * (max_intervals + 1);
  const int a = iv[k], b = iv[k + 1];
  if (a < 0 || b < a || b > len || b - a >= JPEG_MAX_INTERVAL) {
    if (t == 0) atomicOr(&status[f], JPEG_ERR_DESC);
    return;
  }
  bool bad = false;
  if (t < ntab) bad = !jpeg_build_table(huff + ((long long)f * JPEG_MAX_PER_MCU + t) * JPEG_TABLE_BYTES, &tab[t]);
  if (t >= 64 && t < 128) zz[t - 64] = (uint8_t)jpeg_zigzag(t - 64);
  if (__syncthreads_or(bad)) {
    if (t == 0) atomicOr(&status[f], JPEG_ERR_TABLE);
    return;
  }
  const JpegScan sc{comp + s0 + a, b - a, per, hv, tab, zz};
  const int nbits = 8 * (b - a), sb = subseq_bits;
  const int nsub = (int)(((long long)nbits + sb - 1) / sb);
  const int left = mcus - k * r;
  const int limit = (left < r ? left : r) * per;
  const long long nblocks = (long long)mcus * per, base = (long long)k * r * per;
  int16_t* __restrict__ fb = blocks + (long long)f * nblocks * 64;
  int cp = 0, cbz = 0, err = 0, most = 0;                            // the chunk's first state; cn, cdc: the interval's totals so far
  unsigned cn = 0, cdc[3] = {0, 0, 0};
  for (int c0 = 0; c0 < nsub; c0 += JPEG_WG) {
    const int na = nsub - c0 < JPEG_WG ? nsub - c0 : JPEG_WG;
    const bool active = t < na;
    const long long e64 = (long long)(c0 + t + 1) * sb;
    const int send = e64 < nbits ? (int)e64 : nbits;
    // phase 1
    int my_p = t == 0 ? cp : (active ? (c0 + t) * sb : 0), my_bz = t == 0 ? cbz : 0;
    JpegState ex = jpeg_fresh(my_p, my_bz);
    if (active) {
      jpeg_decode_span<false>(sc, ex, send, nullptr, 0, 0, 0, nullptr);
      ex_p[t] = ex.p, ex_bz[t] = (ex.b << 8) | ex.z;
    }
    __syncthreads();
    // phase 2: at most na - 1 rounds
    int used = 0;
    for (int round = 1; round < na; ++round) {
      bool changed = false;
      if (active && t > 0) {
        const int pp = ex_p[t - 1], pbz = ex_bz[t - 1];
        if (pp != my_p || pbz != my_bz) {
          changed = true, my_p = pp, my_bz = pbz;
          ex = jpeg_fresh(pp, pbz);
          jpeg_decode_span<false>(sc, ex, send, nullptr, 0, 0, 0, nullptr);
        }
      }
      const int any = __syncthreads_or(changed);                     // every exit of the round before has been read
      ++used;
      if (!any) break;
      if (changed) ex_p[t] = ex.p, ex_bz[t] = (ex.b << 8) | ex.z;
      __syncthreads();
    }
    most = used > most ? used : most;
    // phase 3
    unsigned tn, tdc[3] = {0, 0, 0}, xdc[3] = {0, 0, 0};
    const unsigned xn = jpeg_scan(active ? (unsigned)ex.n : 0u, wave_tot, &tn);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c <= per - hv) xdc[c] = jpeg_scan(active ? (unsigned)ex.dc[c] : 0u, wave_tot, &tdc[c]);   // (uniform: a scan per component)
    if (active) {
      const long long owed = (long long)limit - (long long)(cn + xn);
      if (owed > 0) {
        const int pred[3] = {(int)(cdc[0] + xdc[0]), (int)(cdc[1] + xdc[1]), (int)(cdc[2] + xdc[2])};
        JpegState w = jpeg_fresh(my_p, my_bz);
        jpeg_decode_span<true>(sc, w, send, fb, nblocks, base + (long long)(cn + xn), (int)owed, pred);
        err |= w.err;
      }
    }
    cp = ex_p[na - 1], cbz = ex_bz[na - 1];
    cn += tn;
#pragma unroll
    for (int c = 0; c < 3; ++c) cdc[c] += tdc[c];
    if (cn > (1u << 30)) cn = 1u << 30;                              // (more blocks than any frame has: only the comparison with `limit` matters)
    __syncthreads();                                                 // the exits are read before the next chunk writes its own
  }
  if (t == 0 && (long long)cn < limit) err |= JPEG_ERR_EXHAUSTED;
  if (err) atomicOr(&status[f], err);
  if (t == 0) atomicMax(&rounds[f], most);
}

// jidctint.c's one-dimensional pass, modulo 2^32
__device__ __forceinline__ void jpeg_idct_pass(const int (&in)[8], int (&out)[8], int shift) {
  typedef unsigned U;
  const U c0 = (U)in[0], c1 = (U)in[1], c2 = (U)in[2], c3 = (U)in[3], c4 = (U)in[4], c5 = (U)in[5], c6 = (U)in[6], c7 = (U)in[7];
  U z1 = (c2 + c6) * 4433u;
  const U tmp2 = z1 - c6 * 15137u, tmp3 = z1 + c2 * 6270u;
  const U tmp0 = (c0 + c4) << 13, tmp1 = (c0 - c4) << 13;
  const U t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  U o0 = c7, o1 = c5, o2 = c3, o3 = c1;
  z1 = o0 + o3;
  U z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const U z5 = (z3 + z4) * 9633u;
  o0 *= 2446u, o1 *= 16819u, o2 *= 25172u, o3 *= 12299u;
  z1 *= (U)-7373, z2 *= (U)-20995, z3 = z3 * (U)-16069 + z5, z4 = z4 * (U)-3196 + z5;
  o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
  const U half = 1u << (shift - 1);
  out[0] = (int)(t10 + o3 + half) >> shift, out[7] = (int)(t10 - o3 + half) >> shift;
  out[1] = (int)(t11 + o2 + half) >> shift, out[6] = (int)(t11 - o2 + half) >> shift;
  out[2] = (int)(t12 + o1 + half) >> shift, out[5] = (int)(t12 - o1 + half) >> shift;
  out[3] = (int)(t13 + o0 + half) >> shift, out[4] = (int)(t13 - o0 + half) >> shift;
}

struct JpegGeom {
  int W, H, ncomp, h, v, mx, my, per, hv;
  long long y_bytes, c_bytes, plane_bytes;                           // luma plane, one chroma plane, all planes of a file
};

__host__ __device__ inline JpegGeom jpeg_geom(int W, int H, int ncomp, int h, int v) {
  JpegGeom g;
  g.W = W, g.H = H, g.ncomp = ncomp, g.h = h, g.v = v;
  g.mx = (W + 8 * h - 1) / (8 * h), g.my = (H + 8 * v - 1) / (8 * v);
  g.hv = h * v, g.per = ncomp == 3 ? h * v + 2 : 1;
  g.y_bytes = (long long)g.my * v * 8 * g.mx * h * 8;
  g.c_bytes = ncomp == 3 ? (long long)g.my * 8 * g.mx * 8 : 0;
  g.plane_bytes = g.y_bytes + 2 * g.c_bytes;
  return g;
}

constexpr int JPEG_IDCT_THREADS = 256;

__global__ __launch_bounds__(JPEG_IDCT_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ blocks, const uint16_t* __restrict__ quant,
                                                                      JpegGeom g, uint8_t* __restrict__ planes, int* __restrict__ status) {
  __shared__ int ws[JPEG_IDCT_THREADS / 8][8][9];
  const int f = blockIdx.y, t = threadIdx.x, j = t & 7, slot = t >> 3;
  if (status[f] & ~JPEG_ERR_RANGE) return;                           // (uniform: the entropy launches' answer)
  const long long nblocks = (long long)g.mx * g.my * g.per;
  const long long blk = (long long)blockIdx.x * (JPEG_IDCT_THREADS / 8) + slot;
  const bool active = blk < nblocks;
  int comp = 0, row0 = 0, col0 = 0, pitch = g.mx * g.h * 8;
  long long plane0 = 0;
  bool bad = false;
  if (active) {
    const int mcu = (int)(blk / g.per), b = (int)(blk % g.per), mcu_y = mcu / g.mx, mcu_x = mcu % g.mx;
    if (b < g.hv) {
      row0 = (mcu_y * g.v + b / g.h) * 8, col0 = (mcu_x * g.h + b % g.h) * 8;
    } else {
      comp = 1 + b - g.hv, row0 = mcu_y * 8, col0 = mcu_x * 8, pitch = g.mx * 8;
      plane0 = g.y_bytes + (comp - 1) * g.c_bytes;
    }
    const int16_t* __restrict__ cf = blocks + ((long long)f * nblocks + blk) * 64;
    const uint16_t* __restrict__ q = quant + ((long long)f * 3 + comp) * 64;
    int in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      in[r] = (int)cf[r * 8 + j] * (int)q[r * 8 + j];
      bad |= in[r] > 32767 || in[r] < -32767;
    }
    jpeg_idct_pass(in, out, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      bad |= out[r] > 32767 || out[r] < -32768;
      ws[slot][r][j] = out[r];
    }
  }
  __syncthreads();
  if (active) {
    int in[8], out[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) in[c] = ws[slot][j][c];
    jpeg_idct_pass(in, out, 18);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      bad |= out[c] > 511 || out[c] < -512;
      int p = out[c] + 128;
      p = p < 0 ? 0 : (p > 255 ? 255 : p);
      if (c < 4) lo |= (unsigned)p << (8 * c);
      else hi |= (unsigned)p << (8 * (c - 4));
    }
    // row0 + j < the plane's rows and col0 + 8 <= pitch by construction: the planes are whole MCUs
    uint2* dst = reinterpret_cast<uint2*>(planes + (long long)f * g.plane_bytes + plane0 + (long long)(row0 + j) * pitch + col0);
    *dst = make_uint2(lo, hi);
  }
  if (__syncthreads_or(bad) && t == 0) atomicOr(&status[f], JPEG_ERR_RANGE);
}

constexpr int JPEG_COLOUR_THREADS = 256;

__device__ __forceinline__ int jpeg_clamp8(int x) { return x < 0 ? 0 : (x > 255 ? 255 : x); }

// The chroma sample of plane `c` (pitch cp, extent dw x dh) that fancy upsampling gives pixel (y, x)
__device__ __forceinline__ int jpeg_chroma(const uint8_t* __restrict__ c, int cp, int dw, int dh, int h, int v, int y, int x) {
  if (h == 1) return c[(long long)y * cp + x];
  const int cx = x >> 1, odd = x & 1;
  int nx = odd ? cx + 1 : cx - 1;
  nx = nx < 0 ? 0 : (nx > dw - 1 ? dw - 1 : nx);
  if (v == 1) {
    const uint8_t* row = c + (long long)y * cp;
    return (3 * row[cx] + row[nx] + (odd ? 2 : 1)) >> 2;
  }
  const int cy = y >> 1;
  int ny = (y & 1) ? cy + 1 : cy - 1;
  ny = ny < 0 ? 0 : (ny > dh - 1 ? dh - 1 : ny);
  const uint8_t* r0 = c + (long long)cy * cp;
  const uint8_t* r1 = c + (long long)ny * cp;
  const int s = 3 * r0[cx] + r1[cx], sn = 3 * r0[nx] + r1[nx];
  return (3 * s + sn + (odd ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(JPEG_COLOUR_THREADS) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, JpegGeom g, int N,
                                                                          uint8_t* __restrict__ out, const int* __restrict__ status) {
  __shared__ unsigned stage[JPEG_COLOUR_THREADS * 3 / 4];
  uint8_t* sbytes = reinterpret_cast<uint8_t*>(stage);
  const int t = threadIdx.x;
  const long long hw = (long long)g.H * g.W, total = hw * N;         // (3 total < 2^31: the entry's bound)
  const long long px = (long long)blockIdx.x * JPEG_COLOUR_THREADS + t;
  int r = 0, gr = 0, b = 0;
  if (px < total) {
    const int f = (int)(px / hw), i = (int)(px % hw), y = i / g.W, x = i % g.W;
    if (status[f] == JPEG_OK) {                                      // (else the file's pixels are unspecified: zeros)
      const uint8_t* __restrict__ p = planes + (long long)f * g.plane_bytes;
      const int yy = p[(long long)y * (g.mx * g.h * 8) + x];
      if (g.ncomp == 1) {
        r = gr = b = yy;
      } else {
        const int dw = (g.W + g.h - 1) / g.h, dh = (g.H + g.v - 1) / g.v, cp = g.mx * 8;
        const int cb = jpeg_chroma(p + g.y_bytes, cp, dw, dh, g.h, g.v, y, x) - 128;
        const int cr = jpeg_chroma(p + g.y_bytes + g.c_bytes, cp, dw, dh, g.h, g.v, y, x) - 128;
        r = jpeg_clamp8(yy + ((91881 * cr + 32768) >> 16));
        gr = jpeg_clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
        b = jpeg_clamp8(yy + ((116130 * cb + 32768) >> 16));
      }
    }
  }
  sbytes[3 * t] = (uint8_t)r, sbytes[3 * t + 1] = (uint8_t)gr, sbytes[3 * t + 2] = (uint8_t)b;
  __syncthreads();
  // the workgroup's bytes start at a multiple of 768: whole dwords while they last, bytes for the tensor's tail
  const long long byte0 = (long long)blockIdx.x * JPEG_COLOUR_THREADS * 3, bytes = 3 * total;
  if (t < JPEG_COLOUR_THREADS * 3 / 4) {
    const long long at = byte0 + 4LL * t;
    if (at + 4 <= bytes) {
      reinterpret_cast<unsigned*>(out)[at >> 2] = stage[t];
    } else {
      for (int k = 0; k < 4; ++k)
        if (at + k < bytes) out[at + k] = sbytes[4 * t + k];
    }
  }
}

int jpeg_decode(const unsigned char* src, const long long* src_off, const int* ri, const unsigned char* huff, const unsigned short* quant, int N,
                int W, int H, int ncomp, int h, int v, int subseq_bits, int max_intervals, long long src_total, int phases, unsigned char* comp,
                int* ivl, short* blocks, unsigned char* planes, unsigned char* out, int* status, int* rounds, hipStream_t st) {
  const bool sampling = (ncomp == 1 && h == 1 && v == 1) || (ncomp == 3 && ((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2)));
  if (!sampling || W < 16 || H < 16 || W > 16384 || H > 16384 || subseq_bits < 32 || subseq_bits % 32 || subseq_bits > (1 << 20) ||
      max_intervals > (1 << 20) || src_total >= (1LL << 31) || 3LL * N * H * W >= (1LL << 31) || (reinterpret_cast<uintptr_t>(out) & 3) ||
      (reinterpret_cast<uintptr_t>(planes) & 7))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  const JpegGeom g = jpeg_geom(W, H, ncomp, h, v);
  const long long nblocks = (long long)g.mx * g.my * g.per;
  if (N * nblocks * 128 >= (1LL << 40) || (g.plane_bytes & 7)) return UNIVS_ERR_NOT_IMPLEMENTED;
  const int mcus = g.mx * g.my;
  if (phases & 1) {
    if (hipMemsetAsync(status, 0, sizeof(int) * N, st) != hipSuccess || hipMemsetAsync(rounds, 0, sizeof(int) * N, st) != hipSuccess ||
        hipMemsetAsync(blocks, 0, (size_t)(N * nblocks * 128), st) != hipSuccess) {
      (void)hipGetLastError();
      set_error("jpeg_decode: clearing the status and the block buffer failed");
      return UNIVS_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(jpeg_unstuff_kernel, dim3((unsigned)N), dim3(JPEG_UNSTUFF_THREADS), 0, st, src, src_off, ri, src_total, mcus, max_intervals,
                       comp, ivl, status);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)max_intervals, (unsigned)N), dim3(JPEG_WG), 0, st, comp, src_off, ri, huff, ivl,
                       src_total, mcus, g.per, g.hv, 2 * ncomp, subseq_bits, max_intervals, blocks, status, rounds);
  }
  if (phases & 2) {
    const unsigned per_wg = JPEG_IDCT_THREADS / 8;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((nblocks + per_wg - 1) / per_wg), (unsigned)N), dim3(JPEG_IDCT_THREADS), 0, st, blocks,
                       quant, g, planes, status);
    const long long total = (long long)N * H * W;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((total + JPEG_COLOUR_THREADS - 1) / JPEG_COLOUR_THREADS)), dim3(JPEG_COLOUR_THREADS), 0,
                       st, planes, g, N, out, status);
  }
  return check_launch("jpeg_decode");
}

}  // namespace univs
