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
// The building blocks (plane descriptor, taps of the second resize, histogram, grids) and the video_stats / video_instance_masks
// kernels, which are the image ones with other template arguments, are in mask_post.h.
#include "mask_post.h"
#include "launchers.h"

namespace univs {

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
  hist_zero(hist, K);
  const long long ohw = (long long)H0 * W0, n = ohw * pl.V;
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
      hist_covered(hist, k, valid && cov);
    }
    if (valid && id >= 0 && id < K) {
      atomicAdd(&hist[3 * id], 1);
      if (both) atomicAdd(&hist[3 * id + 2], 1);
    }
  }
  hist_flush(hist, K, counts);
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
  hipLaunchKernelGGL(plane_stats_kernel<false>, dim3((unsigned)segs, (unsigned)K), dim3(256), 0, st, make_planes(M, Q, V, h, w, Hp, Wp),
                     rows, step, hi, wi, hi, wi, rps, counts);
  return check_launch("video_mask_stats_f32");
}

int video_instance_masks_u8(const float* M, int Q, int V, int h, int w, int Hp, int Wp, int hi, int wi, const int* rows, int N, int H0,
                            int W0, unsigned char* masks, hipStream_t st) {
  if ((long long)N * V > 65535) return UNIVS_ERR_NOT_IMPLEMENTED;
  int rps = 0;
  const int segs = row_segments(H0, (long long)N * V, &rps);
  hipLaunchKernelGGL(instance_masks_kernel<false>, dim3((unsigned)segs, (unsigned)(N * V)), dim3(256), 0, st,
                     make_planes(M, Q, V, h, w, Hp, Wp), hi, wi, rows, H0, W0, (float)hi / (float)H0, (float)wi / (float)W0, rps, masks,
                     (int*)nullptr);
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
