// The zlib streams of result PNGs, from the id maps (include/univs_png_hip.h).  The four writers of inference/results.py end in
// `PIL.Image.save`, zlib level 6 on one host core per frame; here the device emits each frame's complete zlib stream and the host only
// wraps it in chunks.  The format is stated once, in numpy, in univs_amd/inference/png_rule.py: filtered rows (filter "None"), per row
// the runs of bytes equal to the byte d = C places before as matches of at most 258, everything else as literals, RFC 1951's fixed
// Huffman code, R rows per deflate block, an empty stored block after each so that blocks end on a byte and concatenate.  The bytes
// of that file are the contract; this file restates nothing of it but the code tables, in closed form.
//
// png_stripe_kernel, one workgroup of 256 threads per (stripe, frame).  LDS: the stripe's n <= 24 KB filtered bytes (the look-up
// lut[clamp(id)] is applied while they are formed: no pixel plane exists in memory), the bit buffer of stripe_capacity(n) bytes as
// 32-bit words, 256 words of scan space: at most 52.3 KB, dynamic, sized by the frame's R row_len.  The fill takes the stripe's ids,
// which are consecutive in memory, PNG_FILL per thread and round with their loads issued together.  A thread then owns ceil(n / 256)
// consecutive positions.  (1) It notes the first and last position of its piece where eq is false; an exclusive prefix maximum and an
// exclusive suffix minimum over the threads give every thread the last such position before and the first one after its piece: the
// run start and the run end of any position follow from those and the piece itself (eq is false at a row's first d bytes, so runs end
// at row starts by themselves).  (2) It walks its piece and adds up the bits of its tokens from the closed form; an exclusive sum
// over the threads places it in the stripe's bit stream.  (3) It walks again and ORs each code into the bit buffer: a code is at most
// 18 bits, so at most two words, with LDS atomics because neighbouring threads share words.  Then the block tail, the copy to the
// stripe's slot of `scratch` (byte stores: a slot is exactly stripe_capacity(R row_len) bytes and has no alignment), and the stripe's
// size and Adler partial sums (sum x, sum (n - i) x; reduced mod 65521 per thread, 32-bit sums cannot overflow at n <= 24 KB).
// png_frames_kernel, one workgroup: per frame the stream's length and Adler-32 (a = a1 + a2 - 1, b = b1 + b2 + len2 (a1 - 1)), then
// the running sum into `offsets`.  png_place_kernel, one workgroup per (stripe, frame): the stripe's place from the sizes before it
// in its frame, the copy, the stream's 78 01 by the first and 03 00 + Adler-32 by the last stripe's workgroup.
// Integer only.  Nothing about speed is claimed here; tools/png_bench.py measures it.
#include <stdint.h>

#include "launchers.h"

namespace univs {

constexpr int PNG_STRIPE_BYTES = 24 * 1024;                        // filtered bytes of a stripe in LDS
constexpr unsigned PNG_ADLER = 65521u;
constexpr int PNG_MAX_MATCH = 258;
constexpr int PNG_FILL = 8;                                        // pixels a thread loads per round of the fill

__host__ __device__ inline long long png_stripe_capacity(long long n) { return (9 * n + 13 + 7) / 8 + 4; }

struct PngMax { __device__ int operator()(int a, int b) const { return max(a, b); } };
struct PngMin { __device__ int operator()(int a, int b) const { return min(a, b); } };
struct PngSum { __device__ int operator()(int a, int b) const { return a + b; } };

// Exclusive scan of v over the 256 threads in the order `idx` (threadIdx.x, or 255 - threadIdx.x for a suffix scan); *total: the
// reduction of all 256.  sc: 256 ints of LDS, free again on return.
template <typename Op>
__device__ int block_scan_exclusive(int v, int idx, int identity, int* sc, Op op, int* total) {
  sc[idx] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int u = idx >= o ? sc[idx - o] : identity;
    __syncthreads();
    v = op(u, v);
    sc[idx] = v;
    __syncthreads();
  }
  const int ex = idx > 0 ? sc[idx - 1] : identity;
  *total = sc[255];
  __syncthreads();
  return ex;
}

// Sum of v over the 256 threads.  sc: 256 long longs of LDS, free again on return.
__device__ long long block_sum_ll(long long v, long long* sc) {
  sc[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sc[threadIdx.x] += sc[threadIdx.x + o];
    __syncthreads();
  }
  const long long r = sc[0];
  __syncthreads();
  return r;
}

// The fixed Huffman code of a literal / length symbol as it enters the LSB-first stream (bit-reversed), and its length.
__device__ __forceinline__ unsigned png_symbol(int sym, int* nbits) {
  unsigned code;
  int nb;
  if (sym < 144) {
    code = 0x30 + sym, nb = 8;
  } else if (sym < 256) {
    code = 0x190 + sym - 144, nb = 9;
  } else if (sym < 280) {
    code = sym - 256, nb = 7;
  } else {
    code = 0xC0 + sym - 280, nb = 8;
  }
  *nbits = nb;
  return __brev(code) >> (32 - nb);
}

// A match of L in [3, 258] at distance d in {1, 3}: length symbol, extra bits, distance code, as one word of at most 18 bits.
// x = L - 3 >= 8 lies in the group e = floor(log2 x) - 2 of four symbols with e extra bits each: symbol 257 + 4 e + (x >> e).
__device__ __forceinline__ unsigned png_match(int L, unsigned dist_bits, int* nbits) {
  const int x = L - 3;
  int sym, e = 0;
  if (L == PNG_MAX_MATCH) {
    sym = 285;
  } else if (x < 8) {
    sym = 257 + x;
  } else {
    e = 29 - __clz(x);                                             // (31 - clz) - 2
    sym = 257 + 4 * e + (x >> e);
  }
  int nb;
  unsigned code = png_symbol(sym, &nb);
  code |= (unsigned)(x & ((1 << e) - 1)) << nb;
  nb += e;
  code |= dist_bits << nb;
  *nbits = nb + 5;
  return code;
}

// The walk over a thread's positions [a, b) of the stripe: the tokens of the closed form.  EMIT false: returns their bits.  EMIT
// true: ORs them into `bitbuf` from bit `bitpos` on.  prev_false + 1 is the start of the run that reaches into the piece, next_false
// the first position >= b where eq is false (n: none).
template <bool EMIT>
__device__ int png_walk(const uint8_t* bytes, int a, int b, int row_len, int d, int prev_false, int next_false, unsigned dist_bits,
                        unsigned* bitbuf, unsigned bitpos) {
  int bits = 0;
  if (a >= b) return 0;
  int col = a % row_len;
  int s = prev_false + 1, e_cur = -1;
  // the three bytes before the cursor stay in registers and the next byte is loaded one step ahead: one LDS load per position, issued
  // before the step that needs it.  (History from before the stripe is never used: col >= d puts i - d inside the row.)
  int h1 = a >= 1 ? bytes[a - 1] : 0, h2 = a >= 2 ? bytes[a - 2] : 0, h3 = a >= 3 ? bytes[a - 3] : 0;
  int x = bytes[a];
  for (int i = a; i < b; ++i) {
    const int x_next = i + 1 < b ? bytes[i + 1] : 0;
    const bool eq = col >= d && x == (d == 1 ? h1 : h3);
    unsigned code = 0;
    int nb = 0;
    if (!eq) {
      s = i + 1;
      code = png_symbol(x, &nb);
    } else {
      if (e_cur <= i) {                                            // the run's end: the first position after i where eq is false
        int j = i + 1, cj = col + 1;
        while (j < b && cj < row_len && bytes[j] == bytes[j - d]) ++j, ++cj;
        e_cur = j < b ? j : next_false;
      }
      const int k = i - s, q = k / PNG_MAX_MATCH;
      const int L = min(PNG_MAX_MATCH, (e_cur - s) - q * PNG_MAX_MATCH);
      if (L < 3)
        code = png_symbol(x, &nb);
      else if (k - q * PNG_MAX_MATCH == 0)
        code = png_match(L, dist_bits, &nb);
    }
    if (EMIT && nb) {
      const unsigned w = bitpos >> 5, sh = bitpos & 31;
      atomicOr(&bitbuf[w], code << sh);
      if (sh + nb > 32) atomicOr(&bitbuf[w + 1], code >> (32 - sh));
      bitpos += nb;
    }
    bits += nb;
    if (++col == row_len) col = 0;
    h3 = h2, h2 = h1, h1 = x, x = x_next;
  }
  return bits;
}

template <typename T>
__global__ __launch_bounds__(256) void png_stripe_kernel(const T* __restrict__ src, const uint8_t* __restrict__ lut, int K, int C, int H, int W,
                                                         int R, int S, long long slot, int* __restrict__ meta, uint8_t* __restrict__ slots) {
  extern __shared__ unsigned png_lds[];
  const int t = threadIdx.x;
  const int blk = blockIdx.x, f = blk / S, s = blk - f * S;
  const int row_len = W * C + 1;
  const int y0 = s * R, rows = min(R, H - y0);
  const int n = rows * row_len;                                    // <= PNG_STRIPE_BYTES
  const int cap_words = (int)((png_stripe_capacity(n) + 3) >> 2);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(png_lds);
  unsigned* bitbuf = png_lds + ((n + 3) >> 2);
  int* sc = reinterpret_cast<int*>(bitbuf + cap_words);

  // the filtered bytes: 0, then lut[clamp(id)] of the row's pixels.  The stripe's pixels are consecutive in memory; a thread takes
  // PNG_FILL of them per round, 256 apart, and issues their loads (then their table loads) together: the loop is bound by the latency
  // of global memory, not by its width.
  const T* frame = src + ((long long)f * H + y0) * W;
  const int n_px = rows * W;
  for (int r = t; r < rows; r += 256) bytes[r * row_len] = 0;      // (R is the caller's: more than 256 rows when they are short)
  for (int base = t; base < n_px; base += 256 * PNG_FILL) {
    int id[PNG_FILL];
#pragma unroll
    for (int u = 0; u < PNG_FILL; ++u) {
      const int p = base + u * 256;
      id[u] = p < n_px ? (int)frame[p] : 0;
    }
    if (lut) {
#pragma unroll
      for (int u = 0; u < PNG_FILL; ++u) id[u] = min(max(id[u], 0), K - 1);
    }
    if (C == 1) {
      unsigned v[PNG_FILL];
#pragma unroll
      for (int u = 0; u < PNG_FILL; ++u) v[u] = lut ? (unsigned)lut[id[u]] : ((unsigned)id[u] & 255u);
#pragma unroll
      for (int u = 0; u < PNG_FILL; ++u) {
        const int p = base + u * 256;
        if (p < n_px) bytes[p + p / W + 1] = (uint8_t)v[u];        // row (p / W) starts at row row_len = row (W + 1)
      }
    } else {
      unsigned v[PNG_FILL][3];
#pragma unroll
      for (int u = 0; u < PNG_FILL; ++u) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[u][ch] = lut[3LL * id[u] + ch];
      }
#pragma unroll
      for (int u = 0; u < PNG_FILL; ++u) {
        const int p = base + u * 256;
        if (p < n_px) {
          uint8_t* o = bytes + 3 * p + p / W + 1;
          o[0] = (uint8_t)v[u][0], o[1] = (uint8_t)v[u][1], o[2] = (uint8_t)v[u][2];
        }
      }
    }
  }
  for (int w = t; w < cap_words; w += 256) bitbuf[w] = 0;
  __syncthreads();

  // (1) where eq is false in the thread's piece, and the Adler partial sums
  const int d = C;
  const int per = (n + 255) >> 8;                                  // <= 96
  const int a = min(t * per, n), b = min(a + per, n);
  int last_false = -1, first_false = n;
  unsigned sx = 0, sw = 0;
  if (a < b) {
    int col = a % row_len;
    unsigned h1 = a >= 1 ? bytes[a - 1] : 0, h2 = a >= 2 ? bytes[a - 2] : 0, h3 = a >= 3 ? bytes[a - 3] : 0;
    for (int i = a; i < b; ++i) {
      const unsigned x = bytes[i];
      const unsigned before = d == 1 ? h1 : h3;
      h3 = h2, h2 = h1, h1 = x;
      if (!(col >= d && x == before)) {
        first_false = min(first_false, i);
        last_false = i;
      }
      sx += x;
      sw += (unsigned)(n - i) * x;                                 // <= 96 * 24576 * 255 < 2^32
      if (++col == row_len) col = 0;
    }
  }
  int unused;
  const int prev_false = block_scan_exclusive(last_false, t, -1, sc, PngMax(), &unused);
  const int next_false = block_scan_exclusive(first_false, 255 - t, n, sc, PngMin(), &unused);

  // (2) the bits of the piece's tokens, (3) the codes
  const unsigned dist_bits = d == 1 ? 0u : 8u;                     // the 5-bit codes 0 and 2, reversed
  const int bits = png_walk<false>(bytes, a, b, row_len, d, prev_false, next_false, dist_bits, bitbuf, 0);
  int total;
  const int before = block_scan_exclusive(bits, t, 0, sc, PngSum(), &total);
  png_walk<true>(bytes, a, b, row_len, d, prev_false, next_false, dist_bits, bitbuf, 3u + (unsigned)before);

  // the tail: header bits 0 1 0 at the front; after the tokens 7 zero bits (end of block), 3 zero bits (a stored block, not final),
  // zero bits up to a byte, then LEN = 00 00 and NLEN = FF FF
  const int nbytes = (3 + total + 7 + 3 + 7) / 8 + 4;
  if (t == 0) {
    atomicOr(&bitbuf[0], 2u);
    for (int j = nbytes - 2; j < nbytes; ++j) atomicOr(&bitbuf[j >> 2], 0xFFu << ((j & 3) * 8));
  }
  const int sum_x = block_scan_exclusive((int)(sx % PNG_ADLER), t, 0, sc, PngSum(), &total);
  (void)sum_x;
  const int tot_x = total;
  (void)block_scan_exclusive((int)(sw % PNG_ADLER), t, 0, sc, PngSum(), &total);   // (ends in a barrier: the bit buffer is complete)
  if (t == 0) {
    int* m = meta + 4LL * blk;
    m[0] = nbytes;
    m[1] = (int)((unsigned)tot_x % PNG_ADLER);
    m[2] = (int)((unsigned)total % PNG_ADLER);
    m[3] = 0;
  }
  uint8_t* dst = slots + (long long)blk * slot;
  const uint8_t* from = reinterpret_cast<const uint8_t*>(bitbuf);
  for (int j = t; j < nbytes; j += 256) dst[j] = from[j];
}

// One workgroup.  meta: int32 [N S, 4] = {size, sum x, sum (n - i) x, -}; per frame the stream's length into offsets[f + 1] and its
// Adler-32 into the fourth word of the frame's first stripe, then offsets becomes the running sum.
__global__ __launch_bounds__(256) void png_frames_kernel(int* __restrict__ meta, int N, int S, int H, int R, int row_len,
                                                         long long* __restrict__ offsets) {
  __shared__ long long sc[256];
  const int t = threadIdx.x;
  for (int f = t; f < N; f += 256) {
    int* m = meta + 4LL * f * S;
    long long len = 2 + 2 + 4;
    unsigned long long a = 1, b = 0;
    for (int s = 0; s < S; ++s) {
      len += m[4 * s];
      const unsigned n = (unsigned)(min(R, H - s * R) * row_len);
      const unsigned long long a2 = (1u + (unsigned)m[4 * s + 1]) % PNG_ADLER, b2 = (n + (unsigned)m[4 * s + 2]) % PNG_ADLER;
      b = (b + b2 + (unsigned long long)(n % PNG_ADLER) * ((a + PNG_ADLER - 1) % PNG_ADLER)) % PNG_ADLER;
      a = (a + a2 + PNG_ADLER - 1) % PNG_ADLER;
    }
    m[3] = (int)(unsigned)((b << 16) | a);
    offsets[f + 1] = len;
  }
  __syncthreads();
  const int per = (N + 255) >> 8;
  const int lo = min(t * per, N), hi = min(lo + per, N);
  long long mine = 0;
  for (int f = lo; f < hi; ++f) mine += offsets[f + 1];
  // exclusive sum over the threads: 256 values, by the first thread
  sc[t] = mine;
  __syncthreads();
  if (t == 0) {
    long long run = 0;
    for (int i = 0; i < 256; ++i) {
      const long long v = sc[i];
      sc[i] = run;
      run += v;
    }
    offsets[0] = 0;
  }
  __syncthreads();
  long long run = sc[t];
  for (int f = lo; f < hi; ++f) {
    run += offsets[f + 1];
    offsets[f + 1] = run;
  }
}

__global__ __launch_bounds__(256) void png_place_kernel(const int* __restrict__ meta, int S, long long slot, const uint8_t* __restrict__ slots,
                                                        const long long* __restrict__ offsets, uint8_t* __restrict__ out) {
  __shared__ long long sc[256];
  const int t = threadIdx.x;
  const int blk = blockIdx.x, f = blk / S, s = blk - f * S;
  const int* m = meta + 4LL * f * S;
  long long part = 0;
  for (int k = t; k < s; k += 256) part += m[4 * k];
  const long long before = block_sum_ll(part, sc);
  const int size = m[4 * s];
  uint8_t* base = out + offsets[f];
  uint8_t* dst = base + 2 + before;
  const uint8_t* from = slots + (long long)blk * slot;
  for (int j = t; j < size; j += 256) dst[j] = from[j];
  if (t == 0 && s == 0) {
    base[0] = 0x78;
    base[1] = 0x01;
  }
  if (t == 0 && s == S - 1) {
    const unsigned adler = (unsigned)m[3];
    uint8_t* p = dst + size;
    p[0] = 0x03;
    p[1] = 0x00;
    p[2] = (uint8_t)(adler >> 24);
    p[3] = (uint8_t)(adler >> 16);
    p[4] = (uint8_t)(adler >> 8);
    p[5] = (uint8_t)adler;
  }
}

int png_deflate_maps(const void* src, int src_is_i32, int N, int H, int W, const unsigned char* lut, int K, int C, int rows_per_stripe,
                     unsigned char* scratch, unsigned char* out, long long* offsets, hipStream_t st) {
  const long long row_len = (long long)W * C + 1;
  const int R = rows_per_stripe;
  if ((C != 1 && C != 3) || row_len > PNG_STRIPE_BYTES || R * row_len > PNG_STRIPE_BYTES || (long long)N * H * row_len >= (1LL << 31))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  const int S = (H + R - 1) / R;
  const long long n_full = R * row_len, slot = png_stripe_capacity(n_full);
  const size_t lds = (size_t)(((n_full + 3) >> 2) + ((slot + 3) >> 2) + 256) * 4;      // <= 53.3 KB
  int* meta = reinterpret_cast<int*>(scratch);
  unsigned char* slots = scratch + 16LL * N * S;
  const dim3 grid((unsigned)((long long)N * S));                   // N S <= N H < 2^31
  if (src_is_i32)
    hipLaunchKernelGGL(png_stripe_kernel<int>, grid, dim3(256), lds, st, static_cast<const int*>(src), lut, K, C, H, W, R, S, slot, meta, slots);
  else
    hipLaunchKernelGGL(png_stripe_kernel<unsigned char>, grid, dim3(256), lds, st, static_cast<const unsigned char*>(src), lut, K, C, H, W, R,
                       S, slot, meta, slots);
  hipLaunchKernelGGL(png_frames_kernel, dim3(1), dim3(256), 0, st, meta, N, S, H, R, (int)row_len, offsets);
  hipLaunchKernelGGL(png_place_kernel, grid, dim3(256), 0, st, meta, S, slot, slots, offsets, out);
  return check_launch("png_deflate_maps");
}

}  // namespace univs
