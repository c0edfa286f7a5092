// Video post-processing of the MinVIS-style clip loop (univs/inference/inference_video_vis_fast.py:219-351,
// univs/inference/inference_video_vps.py:209-406) without the per-clip mask list and without the upsampled stack.
//
// The reference keeps every clip's [Q', T, h, w] mask logits in a list until the end of the video, averages each frame over the clips
// that cover it, then resizes all selected masks of all frames to the padded input size ([K, V, Hp, Wp] fp32: ~20 GB at an OVIS-like
// 120-frame video) before it counts, thresholds and resizes again.  Here:
//
//   minvis_accumulate    S[q, i + t] += M[perm[q], t]: the running sum of the clips' masks in the matched order, one writer per element,
//                        clips added in order (the driver scales S to the per-frame mean once, in place, as ATen's mean rounds)
//   video_stats          |U > 1|, |U > -1| over the CROP of frames 0, step, 2 step, ... of each requested row (the quality scores)
//   video_instance_masks bilinear(crop(U) -> H0 x W0) > 0 per frame (a double bilinear: four U taps of four L taps each)
//   video_panoptic_ids   the first-maximum argmax of score_k * sigmoid(U_k) over the kept rows per interim pixel, -1 where no k has
//                        sigmoid(U_k) >= 0.5
//   video_panoptic_counts at the output size: per kept k {|ids == k|, |p_k >= 0.5|, |ids == k and p_k >= 0.5|}, p_k = bilinear(sigmoid(
//                        crop(U_k)) -> H0 x W0), ids resized by ATen's nearest rule (LDS histograms, one set of atomics per workgroup)
//   video_panoptic_paint out = lut[k] where ids == k and p_k >= 0.5, else 0
//
// where U_{q, v} = bilinear(M[q, v] -> Hp x Wp) is evaluated on the fly from the four taps it needs (ATen's source index and term order:
// resample_taps.h) and never written.  M is [Q', V, h, w]; plane (q, v) is q * V + v.  Row and plane indices are clamped on the device.
#include "common.h"
#include "resample_taps.h"

#include <algorithm>

namespace univs {

namespace {

struct Planes {
  const float* M;
  int Q, V, h, w;
  float rh, rw;    // (float) h / Hp, (float) w / Wp: ATen's area_pixel_compute_scale without align_corners
};

__device__ __forceinline__ const float* row_plane(const Planes& pl, const int* __restrict__ rows, int k, int v) {
  int q = rows[k];
  q = q < 0 ? 0 : (q >= pl.Q ? pl.Q - 1 : q);
  return pl.M + ((long long)q * pl.V + v) * ((long long)pl.h * pl.w);
}

__device__ __forceinline__ int wsum_i(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

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

// bilinear(sigmoid(crop(U)) -> H0 x W0) at one output pixel: the resize of the PROBABILITIES (inference_video_vps.py:356-358)
__device__ __forceinline__ float prob_at(const float* plane, int w, const OutTaps& o) {
  return bilerp(o.t2y, o.t2x, sigmoid_f32(u_at(plane, w, o.tya, o.txa)), sigmoid_f32(u_at(plane, w, o.tya, o.txb)),
                sigmoid_f32(u_at(plane, w, o.tyb, o.txa)), sigmoid_f32(u_at(plane, w, o.tyb, o.txb)));
}

// ATen's nearest source index (UpSampleNearest2d.cu): min(floor(dst * (in / out)), in - 1) in fp32
__device__ __forceinline__ int nearest_src(int dst, float scale, int in_size) { return min((int)floorf((float)dst * scale), in_size - 1); }

}  // namespace

// S [Q, V, hw] += M [Qm, T, hw] rows perm[q], frames t < Tv, at frames i + t; VEC = 4: float4 loads and stores (hw % 4 == 0, aligned)
template <int VEC>
__global__ __launch_bounds__(256) void minvis_accumulate_kernel(float* __restrict__ S, const float* __restrict__ M, const int* __restrict__ perm,
                                                                int Q, int Qm, int V, int T, int Tv, int i, long long hwv) {
  const long long total = (long long)Q * Tv * hwv;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long qt = e / hwv, p = e - qt * hwv;
    const int t = (int)(qt % Tv), q = (int)(qt / Tv);
    int src = perm[q];
    src = src < 0 ? 0 : (src >= Qm ? Qm - 1 : src);
    float* d = S + (((long long)q * V + i + t) * hwv + p) * VEC;
    const float* s = M + (((long long)src * T + t) * hwv + p) * VEC;
    if constexpr (VEC == 4) {
      float4 a = *reinterpret_cast<const float4*>(d);
      const float4 b = *reinterpret_cast<const float4*>(s);
      // single-lane adds: kept out of the packed-f32 selection (common.h: fma_single)
      a.x = add_single(a.x, b.x);
      a.y = add_single(a.y, b.y);
      a.z = add_single(a.z, b.z);
      a.w = add_single(a.w, b.w);
      *reinterpret_cast<float4*>(d) = a;
    } else {
      d[0] = add_single(d[0], s[0]);
    }
  }
}

// grid (row segments, K): counts [K, 2] += {|U > 1|, |U > -1|} over rows [y0, y1) of the crop of frames 0, step, 2 step, ...
__global__ __launch_bounds__(256) void video_stats_kernel(Planes pl, int hi, int wi, const int* __restrict__ rows, int step,
                                                          int rows_per_seg, int* __restrict__ counts) {
  const int k = blockIdx.y;
  const int y0 = blockIdx.x * rows_per_seg, y1 = min(hi, y0 + rows_per_seg);
  if (y0 >= y1) return;                                           // (the whole workgroup)
  const int n = (y1 - y0) * wi;
  int c_hi = 0, c_lo = 0;
  for (int v = 0; v < pl.V; v += step) {
    const float* plane = row_plane(pl, rows, k, v);
    for (int e = threadIdx.x; e < n; e += 256) {
      const int r = e / wi, x = e - r * wi, y = y0 + r;
      const float u = u_at(plane, pl.w, make_tap(pl.rh, y, pl.h), make_tap(pl.rw, x, pl.w));
      c_hi += u > 1.f;
      c_lo += u > -1.f;
    }
  }
  c_hi = wsum_i(c_hi);
  c_lo = wsum_i(c_lo);
  __shared__ int part[4][2];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[wave][0] = c_hi;
    part[wave][1] = c_lo;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    c_hi = part[0][0] + part[1][0] + part[2][0] + part[3][0];
    c_lo = part[0][1] + part[1][1] + part[2][1] + part[3][1];
    if (c_hi) atomicAdd(counts + 2 * k, c_hi);
    if (c_lo) atomicAdd(counts + 2 * k + 1, c_lo);
  }
}

// grid (row segments, N V): masks[i, v, oy, ox] = bilinear(crop(U_{rows[i], v}) -> H0 x W0)(oy, ox) > 0
__global__ __launch_bounds__(256) void video_instance_masks_kernel(Planes pl, int hi, int wi, const int* __restrict__ rows, int H0, int W0,
                                                                   float sh, float sw, int rows_per_seg, unsigned char* __restrict__ masks) {
  const int i = blockIdx.y / pl.V, v = blockIdx.y - (blockIdx.y / pl.V) * pl.V;
  const int y0 = blockIdx.x * rows_per_seg, y1 = min(H0, y0 + rows_per_seg);
  if (y0 >= y1) return;
  const float* plane = row_plane(pl, rows, i, v);
  unsigned char* dst = masks + (long long)blockIdx.y * H0 * W0;
  const int n = (y1 - y0) * W0;
#pragma unroll 1
  for (int e = threadIdx.x; e < n; e += 256) {
    const int r = e / W0, ox = e - r * W0, oy = y0 + r;
    const OutTaps o = out_taps(pl, sh, sw, hi, wi, oy, ox);
    const float u = bilerp(o.t2y, o.t2x, u_at(plane, pl.w, o.tya, o.txa), u_at(plane, pl.w, o.tya, o.txb), u_at(plane, pl.w, o.tyb, o.txa),
                           u_at(plane, pl.w, o.tyb, o.txb));
    dst[(long long)oy * W0 + ox] = u > 0.f ? 1 : 0;
  }
}

// ids [V, hi, wi] over the crop: the first k maximising scores[k] * sigmoid(U_k), -1 where every sigmoid(U_k) < 0.5
__global__ __launch_bounds__(256) void video_panoptic_ids_kernel(Planes pl, int hi, int wi, const int* __restrict__ rows,
                                                                 const float* __restrict__ score, int K, int* __restrict__ ids) {
  const long long hw = (long long)hi * wi, n = hw * pl.V;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
    const int v = (int)(p / hw);
    const int r = (int)(p - (long long)v * hw);
    const int y = r / wi, x = r - (r / wi) * wi;
    const Tap ty = make_tap(pl.rh, y, pl.h), tx = make_tap(pl.rw, x, pl.w);
    float best = 0.f;
    int bk = 0;
    bool any = false;
    for (int k = 0; k < K; ++k) {
      const float s = sigmoid_f32(u_at(row_plane(pl, rows, k, v), pl.w, ty, tx));
      const float val = score[k] * s;
      if (k == 0 || val > best) {                                 // argmax(0): the first maximum
        best = val;
        bk = k;
      }
      any |= s >= 0.5f;                                           // is_bg: (sigmoid < 0.5) for every k
    }
    ids[p] = any ? bk : -1;
  }
}

// tiles of 256 output pixels walked by the workgroups in turn (the trip count is uniform over a workgroup: the ballots see every lane);
// counts [K][3] accumulate in LDS and reach global memory once per workgroup
__global__ __launch_bounds__(256) void video_panoptic_counts_kernel(Planes pl, int hi, int wi, const int* __restrict__ rows, int K,
                                                                    const int* __restrict__ ids, int H0, int W0, float sh, float sw,
                                                                    int* __restrict__ counts) {
  extern __shared__ int hist[];                                   // [K][3]: mask_area, original_area, both
  for (int i = threadIdx.x; i < 3 * K; i += 256) hist[i] = 0;
  __syncthreads();
  const long long ohw = (long long)H0 * W0, n = ohw * pl.V;
  const int lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long p = base + threadIdx.x;
    const bool valid = p < n;
    const int v = valid ? (int)(p / ohw) : 0;
    const int r = valid ? (int)(p - (long long)v * ohw) : 0;
    const int oy = r / W0, ox = r - (r / W0) * W0;
    const int id = valid ? ids[((long long)v * hi + nearest_src(oy, sh, hi)) * wi + nearest_src(ox, sw, wi)] : -1;
    const OutTaps o = out_taps(pl, sh, sw, hi, wi, oy, ox);
    bool both = false;
    for (int k = 0; k < K; ++k) {
      const bool cov = prob_at(row_plane(pl, rows, k, v), pl.w, o) >= 0.5f;
      both |= cov && id == k;
      const unsigned long long b = __ballot(valid && cov);
      if (lane == 0 && b) atomicAdd(&hist[3 * k + 1], (int)__popcll(b));
    }
    if (valid && id >= 0 && id < K) {
      atomicAdd(&hist[3 * id], 1);
      if (both) atomicAdd(&hist[3 * id + 2], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * K; i += 256)
    if (hist[i]) atomicAdd(counts + i, hist[i]);
}

// out [V, H0, W0] = lut[k] where the nearest-resized id is k and p_k >= 0.5, else 0
__global__ __launch_bounds__(256) void video_panoptic_paint_kernel(Planes pl, int hi, int wi, const int* __restrict__ rows, int K,
                                                                   const int* __restrict__ ids, const int* __restrict__ lut, int H0, int W0,
                                                                   float sh, float sw, int* __restrict__ out) {
  const long long ohw = (long long)H0 * W0, n = ohw * pl.V;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long long)gridDim.x * 256) {
    const int v = (int)(p / ohw);
    const int r = (int)(p - (long long)v * ohw);
    const int oy = r / W0, ox = r - (r / W0) * W0;
    const int id = ids[((long long)v * hi + nearest_src(oy, sh, hi)) * wi + nearest_src(ox, sw, wi)];
    int o = 0;
    if (id >= 0 && id < K) {
      const int l = lut[id];
      if (l != 0 && prob_at(row_plane(pl, rows, id, v), pl.w, out_taps(pl, sh, sw, hi, wi, oy, ox)) >= 0.5f) o = l;
    }
    out[p] = o;
  }
}

namespace {

Planes make_planes(const float* M, int Q, int V, int h, int w, int Hp, int Wp) {
  return Planes{M, Q, V, h, w, (float)h / (float)Hp, (float)w / (float)Wp};
}

// row segments: enough workgroups to fill the chip (~8 per CU) when there are few planes, at least 8 rows each
int row_segments(int rows, long long planes, int* rows_per_seg) {
  const long long want = (2048 + planes - 1) / planes;
  int segs = (int)std::min<long long>(std::max<long long>(want, 1), std::max(1, rows / 8));
  *rows_per_seg = (rows + segs - 1) / segs;
  return (rows + *rows_per_seg - 1) / *rows_per_seg;
}

unsigned flat_blocks(long long n, long long cap) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, cap)); }

}  // namespace

int minvis_accumulate_f32(float* S, int Q, int V, int h, int w, const float* M, int Qm, int T, const int* perm, int i, hipStream_t st) {
  const int Tv = std::min(T, V - i);
  const long long hw = (long long)h * w;
  const bool vec = hw % 4 == 0 && ((uintptr_t)S % 16) == 0 && ((uintptr_t)M % 16) == 0;
  const long long hwv = vec ? hw / 4 : hw;
  const unsigned blocks = flat_blocks((long long)Q * Tv * hwv, 8192);
  if (vec) hipLaunchKernelGGL(minvis_accumulate_kernel<4>, dim3(blocks), dim3(256), 0, st, S, M, perm, Q, Qm, V, T, Tv, i, hwv);
  else hipLaunchKernelGGL(minvis_accumulate_kernel<1>, dim3(blocks), dim3(256), 0, st, S, M, perm, Q, Qm, V, T, Tv, i, hwv);
  return check_launch("minvis_accumulate_f32");
}

int video_mask_stats_f32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int K, int step,
                         int* counts, hipStream_t st) {
  if (K > 65535 || (long long)((V + step - 1) / step) * hi * wi > INT32_MAX) return UNIVS_ERR_NOT_IMPLEMENTED;
  int rps = 0;
  const int segs = row_segments(hi, K, &rps);
  hipLaunchKernelGGL(video_stats_kernel, dim3((unsigned)segs, (unsigned)K), dim3(256), 0, st, make_planes(M, Q, V, h, w, Hp, Wp), hi, wi,
                     rows, step, rps, counts);
  return check_launch("video_mask_stats_f32");
}

int video_instance_masks_u8(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int N, int H0,
                            int W0, unsigned char* masks, hipStream_t st) {
  if ((long long)N * V > 65535) return UNIVS_ERR_NOT_IMPLEMENTED;
  int rps = 0;
  const int segs = row_segments(H0, (long long)N * V, &rps);
  hipLaunchKernelGGL(video_instance_masks_kernel, dim3((unsigned)segs, (unsigned)(N * V)), dim3(256), 0, st,
                     make_planes(M, Q, V, h, w, Hp, Wp), hi, wi, rows, H0, W0, (float)hi / (float)H0, (float)wi / (float)W0, rps, masks);
  return check_launch("video_instance_masks_u8");
}

int video_panoptic_ids_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, const float* scores,
                           int K, int* ids, hipStream_t st) {
  const long long n = (long long)V * hi * wi;
  hipLaunchKernelGGL(video_panoptic_ids_kernel, dim3(flat_blocks(n, 16384)), dim3(256), 0, st, make_planes(M, Q, V, h, w, Hp, Wp), hi, wi,
                     rows, scores, K, ids);
  return check_launch("video_panoptic_ids_i32");
}

int video_panoptic_counts_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int K,
                              const int* ids, int H0, int W0, int* counts, hipStream_t st) {
  if (K > UNIVS_IMAGE_MAX_KEPT || (long long)V * H0 * W0 > INT32_MAX) return UNIVS_ERR_NOT_IMPLEMENTED;
  const long long n = (long long)V * H0 * W0;
  hipLaunchKernelGGL(video_panoptic_counts_kernel, dim3(flat_blocks(n, 2048)), dim3(256), (size_t)3 * K * sizeof(int), st,
                     make_planes(M, Q, V, h, w, Hp, Wp), hi, wi, rows, K, ids, H0, W0, (float)hi / (float)H0, (float)wi / (float)W0, counts);
  return check_launch("video_panoptic_counts_i32");
}

int video_panoptic_paint_i32(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int K,
                             const int* ids, const int* lut, int H0, int W0, int* out, hipStream_t st) {
  const long long n = (long long)V * H0 * W0;
  hipLaunchKernelGGL(video_panoptic_paint_kernel, dim3(flat_blocks(n, 16384)), dim3(256), 0, st, make_planes(M, Q, V, h, w, Hp, Wp), hi, wi,
                     rows, K, ids, lut, H0, W0, (float)hi / (float)H0, (float)wi / (float)W0, out);
  return check_launch("video_panoptic_paint_i32");
}

}  // namespace univs
