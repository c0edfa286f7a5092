// Per-image post-processing of the mask logits (univs/inference/inference_image_generic_seg.py:214-431) without the upsampled stack.
//
// The reference resizes all Q' mask logits L [Q', h, w] to the padded input size (Hp, Wp) first (:219-224: [333, 1024, 1024] fp32 =
// 1.4 GB at the shipped geometry) and then makes several full-size passes over that stack: the quality counts, sigmoid, score x mask,
// argmax, one `(ids == k).sum()` per segment, the semantic einsum, a second bilinear resize per kept instance.  Every kernel here
// evaluates the upsampled value U_q(y, x) = bilinear(L_q -> Hp x Wp)(y, x) on the fly from the four taps of L it needs (ATen's
// area_pixel_compute_source_index and term order: resample_taps.h), so no kernel writes U:
//
//   image_stats      the quality counts |U > 1|, |U > -1| over the padded plane + the box of {U > 0} over the crop, one pass per plane
//   panoptic_ids     first-maximum argmax of score_k * sigmoid(U_k) over the kept k, the covered bit, per-k [mask_area, original_area,
//                    both] counts (LDS histograms, one set of atomics per workgroup)
//   panoptic_paint   out = covered ? lut[id] : 0 at the original size (nearest, ATen's source index), which segments remain
//   semseg           R[c, p] = sum_q P[q, c] sigmoid(U_q(p)) over the crop, sigmoid planes generated into LDS in the prologue of each
//                    query chunk, exact fp32 fused multiply-adds
//   instance_masks   bilinear(crop(U) -> H0 x W0) > 0 (a double bilinear: four U taps of four L taps each) + the box of the result
//
// Plane indices are clamped to [0, Q') on the device, so a bad index reads a wrong plane, never out of bounds.
#include "common.h"
#include "resample_taps.h"

#include <limits.h>

#include <algorithm>

namespace univs {

namespace {

constexpr int kCovered = 1 << 30;      // panoptic id word: bit 30 = sigmoid(U_id) >= 0.5, bits 0..29 = the kept index k

// the low-resolution plane and its resize to (Hp, Wp)
struct Plane {
  const float* L;
  int h, w;
  float rh, rw;    // (float) h / Hp, (float) w / Wp: ATen's area_pixel_compute_scale without align_corners
};

__device__ __forceinline__ const float* plane_ptr(const float* L, const int* __restrict__ planes, int k, int Q, long long hw) {
  int q = planes[k];
  q = q < 0 ? 0 : (q >= Q ? Q - 1 : q);
  return L + (long long)q * hw;
}

__device__ __forceinline__ int wsum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int wmin(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ int wmax(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
  return v;
}

// the mask_stats record [8] = {count_hi, count_lo, left, top, right, bottom, non-empty, 0}: the four waves of a 256-thread workgroup meet
// in LDS, then ONE set of atomics per workgroup
__device__ __forceinline__ void flush_record(int* __restrict__ o, int hi, int lo, int xmin, int ymin, int xmax, int ymax) {
  hi = wsum(hi);
  lo = wsum(lo);
  xmin = wmin(xmin);
  ymin = wmin(ymin);
  xmax = wmax(xmax);
  ymax = wmax(ymax);
  __shared__ int part[4][6];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[wave][0] = hi; part[wave][1] = lo; part[wave][2] = xmin; part[wave][3] = ymin; part[wave][4] = xmax; part[wave][5] = ymax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      hi += part[k][0];
      lo += part[k][1];
      xmin = min(xmin, part[k][2]);
      ymin = min(ymin, part[k][3]);
      xmax = max(xmax, part[k][4]);
      ymax = max(ymax, part[k][5]);
    }
    if (hi) atomicAdd(o + 0, hi);
    if (lo) atomicAdd(o + 1, lo);
    if (ymax >= 0) {
      atomicMin(o + 2, xmin);
      atomicMin(o + 3, ymin);
      atomicMax(o + 4, xmax);
      atomicMax(o + 5, ymax);
    }
  }
}

}  // namespace

__global__ __launch_bounds__(256) void image_record_init_kernel(int* __restrict__ out, int n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int* o = out + (long long)p * 8;
  o[0] = 0; o[1] = 0; o[2] = INT_MAX; o[3] = INT_MAX; o[4] = -1; o[5] = -1; o[6] = 0; o[7] = 0;
}

// empty box -> zeros (convert_mask_to_box's convention) + the non-empty flag
__global__ __launch_bounds__(256) void image_record_finish_kernel(int* __restrict__ out, int n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  int* o = out + (long long)p * 8;
  const bool ne = o[5] >= o[3];
  if (!ne) { o[2] = 0; o[3] = 0; o[4] = 0; o[5] = 0; }
  o[6] = ne ? 1 : 0;
}

// grid (segments, Q'): rows [y0, y1) of plane q of U; counts over the whole padded plane, the box over the crop
__global__ __launch_bounds__(256) void image_stats_kernel(Plane pl, int Hp, int Wp, int hi, int wi, int rows_per_seg, int* __restrict__ out) {
  const int q = blockIdx.y;
  const int y0 = blockIdx.x * rows_per_seg, y1 = min(Hp, y0 + rows_per_seg);
  if (y0 >= y1) return;                                           // (the whole workgroup)
  const float* plane = pl.L + (long long)q * pl.h * pl.w;
  const int n = (y1 - y0) * Wp;
  int c_hi = 0, c_lo = 0, xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
  for (int e = threadIdx.x; e < n; e += 256) {
    const int r = e / Wp, x = e - r * Wp, y = y0 + r;
    const float v = u_at(plane, pl.w, make_tap(pl.rh, y, pl.h), make_tap(pl.rw, x, pl.w));
    c_hi += v > 1.f;
    c_lo += v > -1.f;
    if (v > 0.f && y < hi && x < wi) {
      xmin = min(xmin, x);
      xmax = max(xmax, x);
      ymin = min(ymin, y);
      ymax = max(ymax, y);
    }
  }
  flush_record(out + (long long)q * 8, c_hi, c_lo, xmin, ymin, xmax, ymax);
}

// tiles of 256 crop pixels, walked by the workgroups of the grid in turn (the trip count is uniform over a workgroup: the ballots below
// see every lane).  counts [K][3] accumulate in LDS and reach global memory once per workgroup.
__global__ __launch_bounds__(256) void panoptic_ids_kernel(Plane pl, int Q, int hi, int wi, const int* __restrict__ planes,
                                                           const float* __restrict__ score, int K, int* __restrict__ ids,
                                                           int* __restrict__ counts) {
  extern __shared__ int hist[];                                   // [K][3]: mask_area, original_area, both
  for (int i = threadIdx.x; i < 3 * K; i += 256) hist[i] = 0;
  __syncthreads();
  const long long hw = (long long)pl.h * pl.w;
  const int n = hi * wi;
  const int lane = threadIdx.x & 63;
  for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
    const int p = base + threadIdx.x;
    const bool valid = p < n;
    const int y = valid ? p / wi : 0, x = valid ? p - (p / wi) * wi : 0;
    const Tap ty = make_tap(pl.rh, y, pl.h), tx = make_tap(pl.rw, x, pl.w);
    float best = 0.f;
    int bk = 0;
    bool bcov = false;
    for (int k = 0; k < K; ++k) {
      const float s = sigmoid_f32(u_at(plane_ptr(pl.L, planes, k, Q, hw), pl.w, ty, tx));
      const float v = score[k] * s;
      const bool cov = s >= 0.5f;                                 // after the sigmoid, as the reference compares
      if (k == 0 || v > best) {                                   // argmax(0): the first maximum
        best = v;
        bk = k;
        bcov = cov;
      }
      const unsigned long long b = __ballot(valid && cov);
      if (lane == 0 && b) atomicAdd(&hist[3 * k + 1], (int)__popcll(b));
    }
    if (valid) {
      ids[p] = bk | (bcov ? kCovered : 0);
      atomicAdd(&hist[3 * bk], 1);
      if (bcov) atomicAdd(&hist[3 * bk + 2], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * K; i += 256)
    if (hist[i]) atomicAdd(counts + i, hist[i]);
}

// out[y, x] = covered ? lut[k] : 0 at the source pixel of ATen's nearest resize (UpSampleNearest2d.cu: min(floor(dst * (in / out)),
// in - 1) in fp32); seen[k] = 1 when k's label reached the output
__global__ __launch_bounds__(256) void panoptic_paint_kernel(const int* __restrict__ ids, int hi, int wi, const int* __restrict__ lut, int K,
                                                             int H0, int W0, float sh, float sw, int* __restrict__ out, int* __restrict__ seen) {
  extern __shared__ int seen_l[];
  for (int i = threadIdx.x; i < K; i += 256) seen_l[i] = 0;
  __syncthreads();
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < (long long)H0 * W0) {
    const int oy = (int)(p / W0), ox = (int)(p - (long long)oy * W0);
    const int sy = min((int)floorf((float)oy * sh), hi - 1), sx = min((int)floorf((float)ox * sw), wi - 1);
    const int v = ids[(long long)sy * wi + sx];
    const int k = min(v & (kCovered - 1), K - 1);
    const int o = (v & kCovered) ? lut[k] : 0;
    out[p] = o;
    if (o) seen_l[k] = 1;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K; i += 256)
    if (seen_l[i]) seen[i] = 1;                                   // (every writer stores the same value)
}

// grid (crop pixels / 64, C / (4 ACC)): wave g of a workgroup owns classes [g ACC, (g + 1) ACC) of the block's class range, lane l
// pixel l of the tile.  Per chunk of 16 queries: the sigmoid planes of the tile [16][64] and the probabilities [16][4 ACC] into LDS,
// then 16 x ACC fused multiply-adds per thread (the probabilities are a wave-wide broadcast).  Queries in ascending order, one rounding
// per term.
template <int ACC>
__global__ __launch_bounds__(256) void semseg_kernel(Plane pl, int Q, int hi, int wi, const int* __restrict__ planes,
                                                     const float* __restrict__ P, int Qs, int C, float* __restrict__ R) {
  constexpr int QC = 16, CB = 4 * ACC;
  __shared__ float S[QC][64];
  __shared__ __attribute__((aligned(16))) float Pl[QC][CB];
  const int n = hi * wi;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int p = blockIdx.x * 64 + lane;
  const int cbase = blockIdx.y * CB;
  const bool valid = p < n;
  const int y = valid ? p / wi : 0, x = valid ? p - (p / wi) * wi : 0;
  const Tap ty = make_tap(pl.rh, y, pl.h), tx = make_tap(pl.rw, x, pl.w);
  const long long hw = (long long)pl.h * pl.w;
  float acc[ACC];
#pragma unroll
  for (int j = 0; j < ACC; ++j) acc[j] = 0.f;
  for (int q0 = 0; q0 < Qs; q0 += QC) {
    __syncthreads();                                              // the previous chunk's reads are done
#pragma unroll
    for (int j = 0; j < QC / 4; ++j) {
      const int qq = g + 4 * j;
      S[qq][lane] = q0 + qq < Qs ? sigmoid_f32(u_at(plane_ptr(pl.L, planes, q0 + qq, Q, hw), pl.w, ty, tx)) : 0.f;
    }
    for (int e = threadIdx.x; e < QC * CB; e += 256) {
      const int qq = e / CB, c = e - qq * CB;
      Pl[qq][c] = (q0 + qq < Qs && cbase + c < C) ? P[(long long)(q0 + qq) * C + cbase + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int qq = 0; qq < QC; ++qq) {
      const float s = S[qq][lane];
      const float4* pr = reinterpret_cast<const float4*>(&Pl[qq][g * ACC]);
#pragma unroll
      for (int j = 0; j < ACC / 4; ++j) {
        const float4 pv = pr[j];
        // single-lane forms: kept out of the packed-f32 selection (common.h: fma_single)
        acc[4 * j + 0] = fma_single(pv.x, s, acc[4 * j + 0]);
        acc[4 * j + 1] = fma_single(pv.y, s, acc[4 * j + 1]);
        acc[4 * j + 2] = fma_single(pv.z, s, acc[4 * j + 2]);
        acc[4 * j + 3] = fma_single(pv.w, s, acc[4 * j + 3]);
      }
    }
  }
  if (!valid) return;
#pragma unroll
  for (int j = 0; j < ACC; ++j) {
    const int c = cbase + g * ACC + j;
    if (c < C) R[(long long)c * n + p] = acc[j];
  }
}

// grid (row segments, N): mask[i, oy, ox] = bilinear(crop(U_planes[i]) -> H0 x W0)(oy, ox) > 0 and the record of that mask's box
__global__ __launch_bounds__(256) void instance_masks_kernel(Plane pl, int Q, int hi, int wi, const int* __restrict__ planes, int H0, int W0,
                                                             float sh, float sw, int rows_per_seg, unsigned char* __restrict__ masks,
                                                             int* __restrict__ boxes) {
  const int i = blockIdx.y;
  const int y0 = blockIdx.x * rows_per_seg, y1 = min(H0, y0 + rows_per_seg);
  if (y0 >= y1) return;
  const long long hw = (long long)pl.h * pl.w;
  const float* plane = plane_ptr(pl.L, planes, i, Q, hw);
  unsigned char* dst = masks + (long long)i * H0 * W0;
  const int n = (y1 - y0) * W0;
  int xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
  // one output pixel per iteration: unrolled, the sixteen gathers of several pixels took all 256 VGPRs (one wave per SIMD)
#pragma unroll 1
  for (int e = threadIdx.x; e < n; e += 256) {
    const int r = e / W0, ox = e - r * W0, oy = y0 + r;
    const Tap t2y = make_tap(sh, oy, hi), t2x = make_tap(sw, ox, wi);      // the second resize: crop (hi, wi) -> (H0, W0)
    const int ya = t2y.i0, yb = t2y.i0 + t2y.di, xa = t2x.i0, xb = t2x.i0 + t2x.di;
    const Tap tya = make_tap(pl.rh, ya, pl.h), tyb = make_tap(pl.rh, yb, pl.h);
    const Tap txa = make_tap(pl.rw, xa, pl.w), txb = make_tap(pl.rw, xb, pl.w);
    const float v = bilerp(t2y, t2x, u_at(plane, pl.w, tya, txa), u_at(plane, pl.w, tya, txb), u_at(plane, pl.w, tyb, txa),
                           u_at(plane, pl.w, tyb, txb));
    const bool m = v > 0.f;
    dst[(long long)oy * W0 + ox] = m ? 1 : 0;
    if (m) {
      xmin = min(xmin, ox);
      xmax = max(xmax, ox);
      ymin = min(ymin, oy);
      ymax = max(ymax, oy);
    }
  }
  flush_record(boxes + (long long)i * 8, 0, 0, xmin, ymin, xmax, ymax);
}

namespace {

Plane make_plane(const float* L, int h, int w, int Hp, int Wp) { return Plane{L, h, w, (float)h / (float)Hp, (float)w / (float)Wp}; }

// row segments: enough workgroups to fill the chip (~8 per CU) when there are few planes, at least 8 rows each
int row_segments(int rows, long long planes, int* rows_per_seg) {
  const long long want = (2048 + planes - 1) / planes;
  int segs = (int)std::min<long long>(std::max<long long>(want, 1), std::max(1, rows / 8));
  *rows_per_seg = (rows + segs - 1) / segs;
  return (rows + *rows_per_seg - 1) / *rows_per_seg;
}

}  // namespace

int image_mask_stats_f32(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, int* out, hipStream_t st) {
  if (Q > 65535) return UNIVS_ERR_NOT_IMPLEMENTED;
  const unsigned nb = (unsigned)((Q + 255) / 256);
  hipLaunchKernelGGL(image_record_init_kernel, dim3(nb), dim3(256), 0, st, out, Q);
  int rps = 0;
  const int segs = row_segments(Hp, Q, &rps);
  hipLaunchKernelGGL(image_stats_kernel, dim3((unsigned)segs, (unsigned)Q), dim3(256), 0, st, make_plane(L, h, w, Hp, Wp), Hp, Wp, hi, wi,
                     rps, out);
  hipLaunchKernelGGL(image_record_finish_kernel, dim3(nb), dim3(256), 0, st, out, Q);
  return check_launch("image_mask_stats_f32");
}

int image_panoptic_ids_f32(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int* planes, const float* scores, int K,
                           int* ids, int* counts, hipStream_t st) {
  if (K > UNIVS_IMAGE_MAX_KEPT) return UNIVS_ERR_NOT_IMPLEMENTED;
  const long long tiles = ((long long)hi * wi + 255) / 256;
  const unsigned blocks = (unsigned)std::min<long long>(tiles, 2048);      // each workgroup flushes its histogram once
  hipLaunchKernelGGL(panoptic_ids_kernel, dim3(blocks), dim3(256), (size_t)3 * K * sizeof(int), st, make_plane(L, h, w, Hp, Wp), Q, hi, wi,
                     planes, scores, K, ids, counts);
  return check_launch("image_panoptic_ids_f32");
}

int image_panoptic_paint_i32(const int* ids, int hi, int wi, const int* lut, int K, int H0, int W0, int* out, int* seen, hipStream_t st) {
  if (K > UNIVS_IMAGE_MAX_KEPT) return UNIVS_ERR_NOT_IMPLEMENTED;
  const long long blocks = ((long long)H0 * W0 + 255) / 256;
  hipLaunchKernelGGL(panoptic_paint_kernel, dim3((unsigned)blocks), dim3(256), (size_t)K * sizeof(int), st, ids, hi, wi, lut, K, H0, W0,
                     (float)hi / (float)H0, (float)wi / (float)W0, out, seen);
  return check_launch("image_panoptic_paint_i32");
}

int image_semseg_f32(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int* planes, const float* P, int Qs, int C,
                     float* R, hipStream_t st) {
  // classes per workgroup 4 ACC: 144 for COCO panoptic (133: 8 % idle lanes), 160 for ADE20k (150) and wider vocabularies (several
  // class chunks along the grid's y)
  const long long tiles = ((long long)hi * wi + 63) / 64;
  const int acc = C <= 144 ? 36 : 40;
  const int cchunks = (C + 4 * acc - 1) / (4 * acc);
  if (cchunks > 65535) return UNIVS_ERR_NOT_IMPLEMENTED;
  const dim3 grid((unsigned)tiles, (unsigned)cchunks);
  const Plane pl = make_plane(L, h, w, Hp, Wp);
  if (acc == 36) hipLaunchKernelGGL(semseg_kernel<36>, grid, dim3(256), 0, st, pl, Q, hi, wi, planes, P, Qs, C, R);
  else hipLaunchKernelGGL(semseg_kernel<40>, grid, dim3(256), 0, st, pl, Q, hi, wi, planes, P, Qs, C, R);
  return check_launch("image_semseg_f32");
}

int image_instance_masks_u8(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int* planes, int N, int H0, int W0,
                            unsigned char* masks, int* boxes, hipStream_t st) {
  if (N > 65535) return UNIVS_ERR_NOT_IMPLEMENTED;
  const unsigned nb = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(image_record_init_kernel, dim3(nb), dim3(256), 0, st, boxes, N);
  int rps = 0;
  const int segs = row_segments(H0, N, &rps);
  hipLaunchKernelGGL(instance_masks_kernel, dim3((unsigned)segs, (unsigned)N), dim3(256), 0, st, make_plane(L, h, w, Hp, Wp), Q, hi, wi,
                     planes, H0, W0, (float)hi / (float)H0, (float)wi / (float)W0, rps, masks, boxes);
  hipLaunchKernelGGL(image_record_finish_kernel, dim3(nb), dim3(256), 0, st, boxes, N);
  return check_launch("image_instance_masks_u8");
}

}  // namespace univs
