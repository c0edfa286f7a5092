// Label PNGs read on the device (include/univs_pngread_hip.h): the decoder to png_deflate.hip's encoder, of the general format.  The
// host parses the container (univs_amd/inference/png_read.py) and uploads the zlib streams; two launches turn them into the planes
// the count kernels take.
//
// png_inflate_kernel, one workgroup of one wave per stream.  The serial text (bit reader, block headers, the two Huffman tables,
// symbol decode, every bounds decision) is png_inflate_core.h, the same text tools/png_inflate_host.cpp compiles for the host; every
// lane runs it on the same values, so every branch is uniform.  The tables (built by lane 0) and the last 32 KB of output live in
// LDS: global memory is written only.  Lane j of a match of length L at distance D copies ring[n - D + (j % D)], which is complete
// before the match starts, so overlapping matches need no inner dependency; the barrier in png_match orders the stores of the
// step before ahead of these loads.  The Adler-32 comes from per-lane partial sums, reduced once at the end.
//
// png_unfilter_kernel, one wave per frame, a diagonal wavefront: lane l owns row r0 + l and runs one byte behind lane l - 1, so the
// byte above (b) is what that lane produced in the step before and arrives through one cross-lane shuffle; c is the b of bpp steps
// ago and a the lane's own result of bpp steps ago, both in registers.  All five filter types are one path,
// recon = filt + png_predict(type, a, b, c).  The last row of a group of 64 stays in LDS (PNG_ROW_CAP bytes) for lane 0 of the next
// group: lane 0 reads byte x in step x, lane 63 overwrites it in step x + 63.  The filtered bytes of 8 steps are loaded together, ahead
// of the 8 dependent steps; a lane walks its own row, so its loads hit the lines it has just touched.  The same pass unpacks 1 / 2 /
// 4-bit palette rows (MSB first) and writes [H, W] (indices, grey) or [H, W, 3] (RGB as stored, grey replicated, palette looked up).
// `filtered` is only read here: it keeps the inflated bytes.
//
// Every store is checked against the frame's own region first: png_put's callers against `expect`, the unfilter's against out_bytes;
// both regions are checked against the buffers' sizes when the frame's plan is made.  Nothing about speed is claimed here;
// tools/png_read_bench.py measures it.
#include <stdint.h>

#include "launchers.h"
#include "png_inflate_core.h"

namespace univs {

struct PngWave {
  static constexpr int N = 64;
  static __device__ __forceinline__ int lane() { return (int)threadIdx.x; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};

// The frame's plan and regions; false (and *st = PNG_ERR_DESC) where the descriptor or an offset is not admissible
struct PngFrame {
  PngPlan p;
  long long in0, in1, filt0, out0;
};

__device__ bool png_frame(int f, const long long* __restrict__ stream_offsets, const int* __restrict__ desc, int P,
                          const long long* __restrict__ filt_offsets, const long long* __restrict__ out_offsets, long long streams_total,
                          long long filt_total, long long out_total, int max_rowbytes, PngFrame* fr) {
  fr->p = png_plan(desc + (long long)PNG_DESC * f, P, max_rowbytes);
  fr->in0 = stream_offsets[f], fr->in1 = stream_offsets[f + 1];
  fr->filt0 = filt_offsets[f], fr->out0 = out_offsets[f];
  const long long filt1 = filt_offsets[f + 1], out1 = out_offsets[f + 1];
  return fr->p.ok && fr->in0 >= 0 && fr->in0 <= fr->in1 && fr->in1 <= streams_total && fr->filt0 >= 0 && filt1 <= filt_total &&
         fr->p.expect <= filt1 - fr->filt0 && fr->out0 >= 0 && out1 <= out_total && fr->p.out_bytes <= out1 - fr->out0;
}

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ streams, const long long* __restrict__ stream_offsets,
                                                         const int* __restrict__ desc, int P, const long long* __restrict__ filt_offsets,
                                                         const long long* __restrict__ out_offsets, long long streams_total,
                                                         long long filt_total, long long out_total, int max_rowbytes,
                                                         uint8_t* __restrict__ filtered, int* __restrict__ status) {
  __shared__ uint8_t ring[PNG_WINDOW];
  __shared__ PngTables tables;
  __shared__ unsigned long long red[64];
  const int f = blockIdx.x;
  PngFrame fr;
  int st = PNG_ERR_DESC;
  if (png_frame(f, stream_offsets, desc, P, filt_offsets, out_offsets, streams_total, filt_total, out_total, max_rowbytes, &fr)) {
    st = png_inflate<PngWave>(streams, fr.in0, fr.in1, filtered + fr.filt0, fr.p.expect, ring, &tables, red, nullptr);
  }
  if (threadIdx.x == 0) status[f] = st;
}

// One reconstructed byte of row `row` at byte x of the row, to the frame's plane
__device__ __forceinline__ void png_emit(const PngPlan& p, const uint8_t* __restrict__ pal, uint8_t* __restrict__ o, int row, int x, unsigned r) {
  if (p.bd == 8) {
    if (p.och == (p.ct == 2 ? 3 : 1)) {                            // bytes as stored
      const long long i = (long long)row * p.rowbytes + x;
      if (i < p.out_bytes) o[i] = (uint8_t)r;
      return;
    }
    const long long i = 3 * ((long long)row * p.W + x);            // grey or palette to RGB
    if (i + 2 >= p.out_bytes) return;
    if (p.ct == 3) {
      const uint8_t* q = pal + 3 * r;
      o[i] = q[0], o[i + 1] = q[1], o[i + 2] = q[2];
    } else {
      o[i] = o[i + 1] = o[i + 2] = (uint8_t)r;
    }
    return;
  }
  const int per = 8 / p.bd;                                        // palette indices of 1, 2 or 4 bits, MSB first
  const unsigned mask = (1u << p.bd) - 1;
  for (int q = 0; q < per; ++q) {
    const int px = x * per + q;
    if (px >= p.W) break;
    const unsigned v = (r >> (8 - p.bd * (q + 1))) & mask;
    const long long i = ((long long)row * p.W + px) * p.och;
    if (i + p.och > p.out_bytes) break;
    if (p.och == 1) {
      o[i] = (uint8_t)v;
    } else {
      const uint8_t* c = pal + 3 * v;
      o[i] = c[0], o[i + 1] = c[1], o[i + 2] = c[2];
    }
  }
}

constexpr int PNG_UNROLL = 8;

__global__ __launch_bounds__(64) void png_unfilter_kernel(const int* __restrict__ desc, const uint8_t* __restrict__ palettes, int P,
                                                          const long long* __restrict__ stream_offsets,
                                                          const long long* __restrict__ filt_offsets, const long long* __restrict__ out_offsets,
                                                          long long streams_total, long long filt_total, long long out_total, int max_rowbytes,
                                                          const uint8_t* __restrict__ filtered, uint8_t* __restrict__ out,
                                                          int* __restrict__ status) {
  __shared__ uint8_t above[PNG_ROW_CAP];                           // the last row of the group before
  const int f = blockIdx.x, l = threadIdx.x;
  if (status[f] != PNG_OK) return;                                 // (uniform: the inflate launch's answer)
  PngFrame fr;
  if (!png_frame(f, stream_offsets, desc, P, filt_offsets, out_offsets, streams_total, filt_total, out_total, max_rowbytes, &fr)) return;
  const PngPlan p = fr.p;
  const uint8_t* __restrict__ filt = filtered + fr.filt0;
  uint8_t* __restrict__ o = out + fr.out0;
  const uint8_t* pal = (p.ct == 3 && p.och == 3) ? palettes + 768LL * p.prow : nullptr;
  const long long stride = 1 + (long long)p.rowbytes;
  const int steps = p.rowbytes + 63;
  const bool wide = p.bpp == 3;
  for (int r0 = 0; r0 < p.H; r0 += 64) {
    const int row = r0 + l;
    const bool active = row < p.H;
    const uint8_t* mine = filt + (long long)row * stride;          // row < H: inside [0, expect)
    const int type = active ? mine[0] : 0;
    if (__any(type > 4)) {
      if (l == 0) status[f] = PNG_ERR_FILTER;
      return;
    }
    unsigned h1 = 0, h2 = 0, h3 = 0, b1 = 0, b2 = 0, b3 = 0, last = 0;
    for (int s0 = 0; s0 < steps; s0 += PNG_UNROLL) {
      unsigned fv[PNG_UNROLL], av[PNG_UNROLL];
#pragma unroll
      for (int k = 0; k < PNG_UNROLL; ++k) {
        const int x = s0 + k - l;
        const bool in = active && x >= 0 && x < p.rowbytes;
        fv[k] = in ? mine[1 + x] : 0;
        av[k] = (in && l == 0 && row > 0) ? above[x] : 0;          // x < rowbytes <= PNG_ROW_CAP
      }
#pragma unroll
      for (int k = 0; k < PNG_UNROLL; ++k) {
        const int x = s0 + k - l;
        unsigned b = (unsigned)__shfl_up((int)last, 1);            // what the lane above made of byte x, one step ago
        if (l == 0) b = av[k];
        if (active && x >= 0 && x < p.rowbytes) {
          const unsigned a = wide ? h3 : h1, c = wide ? b3 : b1;
          const unsigned r = (fv[k] + png_predict(type, a, b, c)) & 255u;
          h3 = h2, h2 = h1, h1 = r;
          b3 = b2, b2 = b1, b1 = b;
          last = r;
          png_emit(p, pal, o, row, x, r);
          if (l == 63) above[x] = (uint8_t)r;
        }
      }
    }
    __syncthreads();                                               // the group's last row is complete before the next group reads it
  }
}

int png_read(const unsigned char* streams, const long long* stream_offsets, const int* desc, const unsigned char* palettes, int P,
             const long long* filt_offsets, const long long* out_offsets, int N, long long streams_total, long long filt_total,
             long long out_total, int max_rowbytes, unsigned char* filtered, unsigned char* out, int* status, hipStream_t st) {
  if (max_rowbytes > PNG_ROW_CAP || filt_total >= (1LL << 31) || out_total >= (1LL << 31) || streams_total >= (1LL << 31))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)N), dim3(64), 0, st, streams, stream_offsets, desc, P, filt_offsets, out_offsets,
                     streams_total, filt_total, out_total, max_rowbytes, filtered, status);
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)N), dim3(64), 0, st, desc, palettes, P, stream_offsets, filt_offsets, out_offsets,
                     streams_total, filt_total, out_total, max_rowbytes, filtered, out, status);
  return check_launch("png_read");
}

}  // namespace univs
