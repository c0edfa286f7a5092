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
// Plane indices are clamped to [0, Q') on the device, so a bad index reads a wrong plane, never out of bounds.  The building blocks
// (plane descriptor with V = 1, record, histogram, grids) and the image_stats / instance_masks kernels, which are the video ones with
// other template arguments, are in mask_post.h.
#include "mask_post.h"
#include "launchers.h"

namespace univs {

constexpr int kCovered = 1 << 30;      // panoptic id word: bit 30 = sigmoid(U_id) >= 0.5, bits 0..29 = the kept index k

// tiles of 256 crop pixels, walked by the workgroups of the grid in turn (the trip count is uniform over a workgroup: the ballots below
// see every lane).  counts [K][3] accumulate in LDS and reach global memory once per workgroup.
__global__ __launch_bounds__(256) void panoptic_ids_kernel(Planes pl, int hi, int wi, const int* __restrict__ planes,
                                                           const float* __restrict__ score, int K, int* __restrict__ ids,
                                                           int* __restrict__ counts) {
  extern __shared__ int hist[];                                   // [K][3]: mask_area, original_area, both
  hist_zero(hist, K);
  const int n = hi * wi;
  for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
    const int p = base + threadIdx.x;
    const bool valid = p < n;
    const int y = valid ? p / wi : 0, x = valid ? p - (p / wi) * wi : 0;
    const Tap ty = make_tap(pl.rh, y, pl.h), tx = make_tap(pl.rw, x, pl.w);
    float best = 0.f;
    int bk = 0;
    bool bcov = false;
    for (int k = 0; k < K; ++k) {
      const float s = sigmoid_f32(u_at(row_plane(pl, planes, k, 0), pl.w, ty, tx));
      const float v = score[k] * s;
      const bool cov = s >= 0.5f;                                 // after the sigmoid, as the reference compares
      if (k == 0 || v > best) {                                   // argmax(0): the first maximum
        best = v;
        bk = k;
        bcov = cov;
      }
      hist_covered(hist, k, valid && cov);
    }
    if (valid) {
      ids[p] = bk | (bcov ? kCovered : 0);
      atomicAdd(&hist[3 * bk], 1);
      if (bcov) atomicAdd(&hist[3 * bk + 2], 1);
    }
  }
  hist_flush(hist, K, counts);
}

// out[y, x] = covered ? lut[k] : 0 at the source pixel of ATen's nearest resize (nearest_src); seen[k] = 1 when k's label reached the
// output
__global__ __launch_bounds__(256) void panoptic_paint_kernel(const int* __restrict__ ids, int hi, int wi, const int* __restrict__ lut, int K,
                                                             int H0, int W0, float sh, float sw, int* __restrict__ out, int* __restrict__ seen) {
  extern __shared__ int seen_l[];
  for (int i = threadIdx.x; i < K; i += 256) seen_l[i] = 0;
  __syncthreads();
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < (long long)H0 * W0) {
    const int oy = (int)(p / W0), ox = (int)(p - (long long)oy * W0);
    const int sy = nearest_src(oy, sh, hi), sx = nearest_src(ox, sw, wi);
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
__global__ __launch_bounds__(256) void semseg_kernel(Planes pl, int hi, int wi, const int* __restrict__ planes,
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
  float acc[ACC];
#pragma unroll
  for (int j = 0; j < ACC; ++j) acc[j] = 0.f;
  for (int q0 = 0; q0 < Qs; q0 += QC) {
    __syncthreads();                                              // the previous chunk's reads are done
#pragma unroll
    for (int j = 0; j < QC / 4; ++j) {
      const int qq = g + 4 * j;
      S[qq][lane] = q0 + qq < Qs ? sigmoid_f32(u_at(row_plane(pl, planes, q0 + qq, 0), pl.w, ty, tx)) : 0.f;
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

int image_mask_stats_f32(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, int* out, hipStream_t st) {
  if (Q > 65535) return UNIVS_ERR_NOT_IMPLEMENTED;
  record_init(out, Q, st);
  int rps = 0;
  const int segs = row_segments(Hp, Q, &rps);
  hipLaunchKernelGGL(plane_stats_kernel<true>, dim3((unsigned)segs, (unsigned)Q), dim3(256), 0, st, make_planes(L, Q, 1, h, w, Hp, Wp),
                     (const int*)nullptr, 1, Hp, Wp, hi, wi, rps, out);
  record_finish(out, Q, st);
  return check_launch("image_mask_stats_f32");
}

int image_panoptic_ids_f32(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int* planes, const float* scores, int K,
                           int* ids, int* counts, hipStream_t st) {
  if (K > UNIVS_IMAGE_MAX_KEPT) return UNIVS_ERR_NOT_IMPLEMENTED;
  const unsigned blocks = flat_blocks((long long)hi * wi, 2048);           // each workgroup flushes its histogram once
  hipLaunchKernelGGL(panoptic_ids_kernel, dim3(blocks), dim3(256), (size_t)3 * K * sizeof(int), st, make_planes(L, Q, 1, h, w, Hp, Wp), hi,
                     wi, planes, scores, K, ids, counts);
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
  const Planes pl = make_planes(L, Q, 1, h, w, Hp, Wp);
  if (acc == 36) hipLaunchKernelGGL(semseg_kernel<36>, grid, dim3(256), 0, st, pl, hi, wi, planes, P, Qs, C, R);
  else hipLaunchKernelGGL(semseg_kernel<40>, grid, dim3(256), 0, st, pl, hi, wi, planes, P, Qs, C, R);
  return check_launch("image_semseg_f32");
}

int image_instance_masks_u8(const float* L, int Q, int h, int w, int Hp, int Wp, int hi, int wi, const int* planes, int N, int H0, int W0,
                            unsigned char* masks, int* boxes, hipStream_t st) {
  if (N > 65535) return UNIVS_ERR_NOT_IMPLEMENTED;
  record_init(boxes, N, st);
  int rps = 0;
  const int segs = row_segments(H0, N, &rps);
  hipLaunchKernelGGL(instance_masks_kernel<true>, dim3((unsigned)segs, (unsigned)N), dim3(256), 0, st, make_planes(L, Q, 1, h, w, Hp, Wp), hi,
                     wi, planes, H0, W0, (float)hi / (float)H0, (float)wi / (float)W0, rps, masks, boxes);
  record_finish(boxes, N, st);
  return check_launch("image_instance_masks_u8");
}

}  // namespace univs
