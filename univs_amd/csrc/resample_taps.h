// Bilinear taps (align_corners = false) shared by the resampling kernels (resample.hip) and the post-processing kernels
// (image_post.hip, video_post.hip): ATen's area_pixel_compute_source_index, h1p / w1p edge handling and the lambda products, term by term.
#pragma once
#include "common.h"

namespace univs {

struct Tap {
  int i0, di;      // first tap, +1 or +0 (last row / column)
  float l0, l1;    // weights
};

__device__ __forceinline__ Tap make_tap(float scale, int dst, int in_size) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  Tap t;
  t.i0 = (int)src;
  t.di = (t.i0 < in_size - 1) ? 1 : 0;
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// l0y (l0x a + l1x b) + l1y (l0x c + l1x d) with the roundings spelled out (three products, three fused multiply-adds): left to the
// compiler's contraction the two kernels of resample.hip rounded the same expression differently
__device__ __forceinline__ float bilerp(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {
  const float top = fmaf(tx.l1, b, tx.l0 * a);
  const float bot = fmaf(tx.l1, d, tx.l0 * c);
  return fmaf(ty.l1, bot, ty.l0 * top);
}

// U(y, x) of one plane [h, w] of L from its taps (the post-processing kernels: image_post.hip, video_post.hip)
__device__ __forceinline__ float u_at(const float* __restrict__ plane, int w, const Tap& ty, const Tap& tx) {
  const float* r0 = plane + (long long)ty.i0 * w;
  const float* r1 = r0 + (long long)ty.di * w;
  return bilerp(ty, tx, r0[tx.i0], r0[tx.i0 + tx.di], r1[tx.i0], r1[tx.i0 + tx.di]);
}

// ATen's sigmoid kernel: 1 / (1 + exp(-x)) in fp32, correctly rounded division
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.f / (1.f + expf(-x)); }

}  // namespace univs
