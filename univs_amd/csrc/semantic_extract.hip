// Semantic extraction: bilinear up-sampling -> crop -> nearest compression of the mask features in ONE gather, gfx950.
//
// Replaces univs/inference/inference_video_semantic_extraction.py:219-238:
//     mask_features = F.interpolate(mask_features, size=interim_size, mode="bilinear", align_corners=False)     [T, C, Hp, Wp]
//     mask_features = mask_features[..., :image_size[0], :image_size[1]]                                        [T, C, Hi, Wi]
//     compression   = F.interpolate(mask_features, size=(hc, wc), mode="nearest")                               [T, C, hc, wc]
// and the `[::t_itv]` the driver applies to the concatenated clips before it saves them.  The reference writes the up-sampled stack
// ([5, 256, 736, 1280] fp32 = 4.8 GB per clip) and keeps one pixel in ratio^2 of it (ratio 32 by default: 1 / 1024).  Here
//     out[k, c, oy, ox] = U[t_first + k t_step, c, sy(oy), sx(ox)]
// where U = bilinear(in -> Hp x Wp) is evaluated at the kept pixels only (make_tap / bilerp of resample_taps.h at scale h / Hp, w / Wp:
// the expression of bilinear_resample_f32_kernel, bit-identical) and (sy, sx) is ATen's nearest source index of the resize of the CROP
// (Hi, Wi) -> (hc, wc): min(floor(dst * (float(Hi) / hc)), Hi - 1), scale and product in fp32 (UpSampleNearest2d.cu:
// nearest_neighbor_compute_source_index).  Frames the temporal ratio drops are never read.
//
// A pure gather with no reuse between planes: a thread owns VEC adjacent output pixels of a row, computes their taps once and loops
// over planes (blockIdx.y), SE_PB planes per trip with all 4 * VEC * SE_PB loads issued before the first use.  At ratio 8 on stride-4 features
// adjacent outputs read adjacent column pairs (nearly every line of the input is touched once); at ratio 32 the reads are sparse
// (one 128-byte line per tap pair) and the launch is small, so every plane gets its own blocks.
#include "common.h"
#include "resample_taps.h"
#include "launchers.h"

namespace univs {

__device__ __forceinline__ int nearest_src(float scale, int dst, int in_size) {
  const int s = (int)floorf((float)dst * scale);
  return s < in_size - 1 ? s : in_size - 1;
}

template <int VEC, int SE_PB>   // SE_PB planes per loop trip (loads in flight: 4 * VEC * SE_PB per thread)
__global__ __launch_bounds__(256) void bilinear_crop_nearest_f32_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int h,
                                                                        int w, float rh, float rw, int Hi, int Wi, int hc, int wc,
                                                                        float nh, float nw, int t_first, int t_step,
                                                                        long long planes /* K * C */) {
  const int wq = wc / VEC;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= hc * wq) return;
  const int oy = q / wq, ox = (q - oy * wq) * VEC;
  const Tap ty = make_tap(rh, nearest_src(nh, oy, Hi), h);
  Tap tx[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) tx[v] = make_tap(rw, nearest_src(nw, ox + v, Wi), w);
  const long long hw = (long long)h * w, ohw = (long long)hc * wc;
  const int row0 = ty.i0 * w, row1 = (ty.i0 + ty.di) * w;
  const long long stride = gridDim.y;
  for (long long p0 = blockIdx.y; p0 < planes; p0 += stride * SE_PB) {
    float a[SE_PB][VEC], b[SE_PB][VEC], c[SE_PB][VEC], d[SE_PB][VEC];
#pragma unroll
    for (int j = 0; j < SE_PB; ++j) {
      long long p = p0 + j * stride;
      p = p < planes ? p : p0;                                   // past the end: re-read plane p0 (in bounds), nothing stored
      const long long k = p / C;
      const float* src = in + ((long long)(t_first + k * t_step) * C + (p - k * C)) * hw;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        a[j][v] = src[row0 + tx[v].i0];
        b[j][v] = src[row0 + tx[v].i0 + tx[v].di];
        c[j][v] = src[row1 + tx[v].i0];
        d[j][v] = src[row1 + tx[v].i0 + tx[v].di];
      }
    }
#pragma unroll
    for (int j = 0; j < SE_PB; ++j) {
      const long long p = p0 + j * stride;
      if (p >= planes) break;
      float o[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = bilerp(ty, tx[v], a[j][v], b[j][v], c[j][v], d[j][v]);
      float* dst = out + p * ohw + (long long)oy * wc + ox;
      if (VEC == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) dst[v] = o[v];
      }
    }
  }
}

// in [T, C, h, w] -> out [K, C, hc, wc] (contiguous; may point into a larger [V', C, hc, wc] buffer).  The caller has checked the
// geometry (capi.hip); UNIVS_ERR_NOT_IMPLEMENTED where a plane does not fit the 32-bit offsets inside the kernel.
int bilinear_crop_nearest_f32(const float* in, float* out, int C, int h, int w, int Hp, int Wp, int Hi, int Wi, int hc, int wc, int t_first,
                              int t_step, int K, hipStream_t st) {
  if ((long long)h * w >= (1LL << 31) || (long long)hc * wc >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  const long long planes = (long long)K * C;
  const float rh = (float)h / (float)Hp, rw = (float)w / (float)Wp;          // as bilinear_resample_f32
  const float nh = (float)Hi / (float)hc, nw = (float)Wi / (float)wc;        // ATen: compute_scales_value<float>(nullopt, in, out)
  const bool vec4 = (wc % 4 == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  const long long groups = (long long)hc * (vec4 ? wc / 4 : wc);
  const long long gx = (groups + 255) / 256;
  if (gx >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  // planes across blockIdx.y.  A small launch (a [5, 256, 22, 40] output: 1280 blocks of 220 threads) gives every plane its own row of
  // blocks so that it spreads over the device; a larger one takes `pb` planes per trip (32 / 16 loads in flight per thread, ~90 VGPRs
  // in the 16-byte form), the rows sized so that the trips come out even.
  const bool small = gx * planes <= 4096;
  const int pb = vec4 ? 2 : 4;
  long long gy = planes;
  if (!small) {
    long long gy_max = 4096 / gx;
    gy_max = gy_max < 1 ? 1 : gy_max;
    const long long trips = (planes + gy_max * pb - 1) / (gy_max * pb);
    gy = (planes + trips * pb - 1) / (trips * pb);
  }
  gy = gy < 65535 ? gy : 65535;
  const dim3 grid((unsigned)gx, (unsigned)gy);
#define SE_LAUNCH(VEC, PB)                                                                                                              \
  hipLaunchKernelGGL((bilinear_crop_nearest_f32_kernel<VEC, PB>), grid, dim3(256), 0, st, in, out, C, h, w, rh, rw, Hi, Wi, hc, wc, nh, nw, \
                     t_first, t_step, planes)
  if (vec4 && small) SE_LAUNCH(4, 1);
  else if (vec4) SE_LAUNCH(4, 2);
  else if (small) SE_LAUNCH(1, 1);
  else SE_LAUNCH(1, 4);
#undef SE_LAUNCH
  return check_launch("bilinear_crop_nearest_f32");
}

}  // namespace univs
