// What the mask post-processing kernels share (mask_stats.hip, image_post.hip, video_post.hip): wave reductions, the 8-int plane record,
// the grid heuristics, the low-resolution plane descriptor, the resized values evaluated on the fly (on top of resample_taps.h), the
// [K][3] LDS histogram, and the two kernels that the image and the video entry points run with different template arguments.
#pragma once
#include "common.h"
#include "resample_taps.h"

#include <limits.h>

#include <algorithm>

namespace univs {

// ---- 64-lane wave reductions --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}

// ---- the plane record ---------------------------------------------------------------------------------------------------------------
// o[8] = {count_hi, count_lo, left, top, right, bottom, non-empty, 0}; corners are inclusive pixel indices, zeros for an empty plane
// (convert_mask_to_box's convention).  record_init before the accumulating kernel, record_finish after it (mask_stats.hip).
void record_init(int* out, long long n, hipStream_t st);
void record_finish(int* out, long long n, hipStream_t st);

// A 256-thread workgroup's part of a record, called by all of its threads.  The four waves meet in LDS: ONE set of atomics per workgroup
// (with one per wave, a plane's ~2 000 atomics on a single cache line took longer than the pass over its pixels when few planes are
// cut into many segments).  COUNTS: o[0:2] += {hi, lo}; BOX: o[2:6] min / max the corners (an untouched box is xmin = ymin = INT_MAX,
// xmax = ymax = -1).
template <bool COUNTS, bool BOX>
__device__ __forceinline__ void flush_record(int* __restrict__ o, int hi, int lo, int xmin, int ymin, int xmax, int ymax) {
  if constexpr (COUNTS) {
    hi = wave_sum(hi);
    lo = wave_sum(lo);
  }
  if constexpr (BOX) {
    xmin = wave_min(xmin);
    ymin = wave_min(ymin);
    xmax = wave_max(xmax);
    ymax = wave_max(ymax);
  }
  __shared__ int part[4][6];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    if constexpr (COUNTS) { part[wave][0] = hi; part[wave][1] = lo; }
    if constexpr (BOX) { part[wave][2] = xmin; part[wave][3] = ymin; part[wave][4] = xmax; part[wave][5] = ymax; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if constexpr (COUNTS) {
        hi += part[k][0];
        lo += part[k][1];
      }
      if constexpr (BOX) {
        xmin = min(xmin, part[k][2]);
        ymin = min(ymin, part[k][3]);
        xmax = max(xmax, part[k][4]);
        ymax = max(ymax, part[k][5]);
      }
    }
    if (COUNTS && hi) atomicAdd(o + 0, hi);
    if (COUNTS && lo) atomicAdd(o + 1, lo);
    if (BOX && ymax >= 0) {
      atomicMin(o + 2, xmin);
      atomicMin(o + 3, ymin);
      atomicMax(o + 4, xmax);
      atomicMax(o + 5, ymax);
    }
  }
}

// ---- grids --------------------------------------------------------------------------------------------------------------------------
// row segments: enough workgroups to fill the chip (~8 per CU) when there are few planes, at least 8 rows each
inline int row_segments(int rows, long long planes, int* rows_per_seg) {
  const long long want = (2048 + planes - 1) / planes;
  int segs = (int)std::min<long long>(std::max<long long>(want, 1), std::max(1, rows / 8));
  *rows_per_seg = (rows + segs - 1) / segs;
  return (rows + *rows_per_seg - 1) / *rows_per_seg;
}

// workgroups of 256 threads over n elements, at most cap of them (the kernel strides)
inline unsigned flat_blocks(long long n, long long cap) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap)); }

// ---- the low-resolution planes M [Q, V, h, w] and their resize to (Hp, Wp); an image is V = 1 ---------------------------------------
struct Planes {
  const float* M;
  int Q, V, h, w;
  float rh, rw;    // (float) h / Hp, (float) w / Wp: ATen's area_pixel_compute_scale without align_corners
};

inline Planes make_planes(const float* M, int Q, int V, int h, int w, int Hp, int Wp) {
  return Planes{M, Q, V, h, w, (float)h / (float)Hp, (float)w / (float)Wp};
}

// plane (q, v); q is clamped to [0, Q), so a bad index reads a wrong plane, never out of bounds
__device__ __forceinline__ const float* plane_at(const Planes& pl, int q, int v) {
  q = q < 0 ? 0 : (q >= pl.Q ? pl.Q - 1 : q);
  return pl.M + ((long long)q * pl.V + v) * ((long long)pl.h * pl.w);
}
__device__ __forceinline__ const float* row_plane(const Planes& pl, const int* __restrict__ rows, int k, int v) {
  return plane_at(pl, rows[k], v);
}

// ---- resized values -----------------------------------------------------------------------------------------------------------------
// ATen's nearest source index (UpSampleNearest2d.cu): min(floor(dst * (in / out)), in - 1) in fp32
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) { return min((int)floorf((float)dst * scale), in_size - 1); }

// the four U taps of an output pixel of the second resize (crop (hi, wi) -> (H0, W0)) and the L taps of each
struct OutTaps {
  Tap t2y, t2x, tya, tyb, txa, txb;
};

__device__ __forceinline__ OutTaps out_taps(const Planes& pl, float sh, float sw, int hi, int wi, int oy, int ox) {
  OutTaps o;
  o.t2y = make_tap(sh, oy, hi);
  o.t2x = make_tap(sw, ox, wi);
  o.tya = make_tap(pl.rh, o.t2y.i0, pl.h);
  o.tyb = make_tap(pl.rh, o.t2y.i0 + o.t2y.di, pl.h);
  o.txa = make_tap(pl.rw, o.t2x.i0, pl.w);
  o.txb = make_tap(pl.rw, o.t2x.i0 + o.t2x.di, pl.w);
  return o;
}

// bilinear(crop(U) -> H0 x W0) at one output pixel: a double bilinear, four U taps of four L taps each
__device__ __forceinline__ float logit_at(const float* plane, int w, const OutTaps& o) {
  return bilerp(o.t2y, o.t2x, u_at(plane, w, o.tya, o.txa), u_at(plane, w, o.tya, o.txb), u_at(plane, w, o.tyb, o.txa),
                u_at(plane, w, o.tyb, o.txb));
}

// bilinear(sigmoid(crop(U)) -> H0 x W0) at one output pixel: the resize of the PROBABILITIES (inference_video_vps.py:356-358)
__device__ __forceinline__ float prob_at(const float* plane, int w, const OutTaps& o) {
  return bilerp(o.t2y, o.t2x, sigmoid_f32(u_at(plane, w, o.tya, o.txa)), sigmoid_f32(u_at(plane, w, o.tya, o.txb)),
                sigmoid_f32(u_at(plane, w, o.tyb, o.txa)), sigmoid_f32(u_at(plane, w, o.tyb, o.txb)));
}

// ---- the LDS histogram [K][3] = {mask_area, original_area, both} of the panoptic kernels --------------------------------------------
// Accumulated in LDS over the tiles a workgroup walks, it reaches global memory once per workgroup.  All three are called by every
// thread of a 256-thread workgroup.
// (the _n forms: a histogram of n cells of any layout -- the count kernels behind count_core.h)
__device__ __forceinline__ void hist_zero_n(int* hist, int n) {
  for (int i = threadIdx.x; i < n; i += 256) hist[i] = 0;
  __syncthreads();
}
__device__ __forceinline__ void hist_zero(int* hist, int K) { hist_zero_n(hist, 3 * K); }

// original_area of k += the lanes of this wave with `covered` set, one LDS atomic per wave (the ballot has to see every lane: the
// caller's trip count is uniform over the workgroup)
__device__ __forceinline__ void hist_covered(int* hist, int k, bool covered) {
  const unsigned long long b = __ballot(covered);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&hist[3 * k + 1], (int)__popcll(b));
}

__device__ __forceinline__ void hist_flush_n(const int* hist, int n, int* __restrict__ counts) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256)
    if (hist[i]) atomicAdd(counts + i, hist[i]);
}
__device__ __forceinline__ void hist_flush(const int* hist, int K, int* __restrict__ counts) { hist_flush_n(hist, 3 * K, counts); }

// ---- the kernels that the image and the video entry points share --------------------------------------------------------------------
// grid (row segments, K): the quality counts {|U > 1|, |U > -1|} of one row of planes over rows [y0, y1) of frames 0, step, 2 step, ...
//   IMAGE:  plane k itself, counts over the padded plane (Hc, Wc) = (Hp, Wp) and the box of {U > 0} over the crop (hi, wi), into the
//           record out[k][8]
//   video:  plane rows[k], counts over the crop (Hc, Wc) = (hi, wi), into out[k][2]
template <bool IMAGE>
__global__ __launch_bounds__(256) void plane_stats_kernel(Planes pl, const int* __restrict__ rows, int step, int Hc, int Wc, int hi, int wi,
                                                          int rows_per_seg, int* __restrict__ out) {
  const int k = blockIdx.y;
  const int y0 = blockIdx.x * rows_per_seg, y1 = min(Hc, y0 + rows_per_seg);
  if (y0 >= y1) return;                                           // (the whole workgroup: no barrier is skipped by a part of it)
  const int n = (y1 - y0) * Wc;
  int c_hi = 0, c_lo = 0, xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
  for (int v = 0; v < (IMAGE ? 1 : pl.V); v += IMAGE ? 1 : step) {      // (an image: its one frame)
    const float* plane = plane_at(pl, IMAGE ? k : rows[k], v);
    for (int e = threadIdx.x; e < n; e += 256) {
      const int r = e / Wc, x = e - r * Wc, y = y0 + r;
      const float u = u_at(plane, pl.w, make_tap(pl.rh, y, pl.h), make_tap(pl.rw, x, pl.w));
      c_hi += u > 1.f;
      c_lo += u > -1.f;
      if (IMAGE && u > 0.f && y < hi && x < wi) {
        xmin = min(xmin, x);
        xmax = max(xmax, x);
        ymin = min(ymin, y);
        ymax = max(ymax, y);
      }
    }
  }
  flush_record<true, IMAGE>(out + (long long)k * (IMAGE ? 8 : 2), c_hi, c_lo, xmin, ymin, xmax, ymax);
}

// grid (row segments, N V): masks[i, v, oy, ox] = bilinear(crop(U_{rows[i], v}) -> H0 x W0)(oy, ox) > 0; BOX: and the record of that
// mask's box into boxes[i V + v][8]
template <bool BOX>
__global__ __launch_bounds__(256) void instance_masks_kernel(Planes pl, int hi, int wi, const int* __restrict__ rows, int H0, int W0,
                                                             float sh, float sw, int rows_per_seg, unsigned char* __restrict__ masks,
                                                             int* __restrict__ boxes) {
  const int i = blockIdx.y / pl.V, v = blockIdx.y - i * pl.V;
  const int y0 = blockIdx.x * rows_per_seg, y1 = min(H0, y0 + rows_per_seg);
  if (y0 >= y1) return;
  const float* plane = row_plane(pl, rows, i, v);
  unsigned char* dst = masks + (long long)blockIdx.y * H0 * W0;
  const int n = (y1 - y0) * W0;
  int xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
  // one output pixel per iteration: unrolled, the sixteen gathers of several pixels took all 256 VGPRs (one wave per SIMD)
#pragma unroll 1
  for (int e = threadIdx.x; e < n; e += 256) {
    const int r = e / W0, ox = e - r * W0, oy = y0 + r;
    const bool m = logit_at(plane, pl.w, out_taps(pl, sh, sw, hi, wi, oy, ox)) > 0.f;
    dst[(long long)oy * W0 + ox] = m ? 1 : 0;
    if (BOX && m) {
      xmin = min(xmin, ox);
      xmax = max(xmax, ox);
      ymin = min(ymin, oy);
      ymax = max(ymax, oy);
    }
  }
  if constexpr (BOX) flush_record<false, true>(boxes + (long long)blockIdx.y * 8, 0, 0, xmin, ymin, xmax, ymax);
}

}  // namespace univs
