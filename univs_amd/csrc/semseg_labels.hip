// The labels of a semantic result without its [C, H, W] tensor, and the confusion matrix of two label maps, gfx950.
//
// The per-image driver's semantic result is bilinear(r [C, hi, wi] -> H x W) (inference/image_generic_seg.py: semantic_inference), and the
// first thing an evaluator does with it is argmax(0): at ADE20K's 150 classes and a 512 x 683 image 210 MB are written and read back for
// 0.35 MB of labels.  semseg_labels_kernel evaluates the resized values where it compares them and writes one byte per pixel.
//
// The compared values carry the bits ops.bilinear_resample would have stored: make_tap / bilerp of resample_taps.h, the scales formed as
// in resample.hip's launcher, this file compiled with resample.hip's flags.  The first maximum wins (strict > while c ascends), which is
// ATen's argmax on finite inputs; the order of NaNs is not specified.
//
// A lane owns four adjacent output pixels of one row: their taps and weights are made once, outside the class loop (the planar kernel
// makes them once per plane), and the two taps of a row come with one 8-byte load.  The four waves of a workgroup hold the SAME 64 pixel groups and a quarter of the classes each, in ascending
// order (wave 0 the first quarter): a 480 x 640 image has 300 workgroups' worth of pixel groups only, and a lane that walks 133 planes
// alone leaves most of the chip's loads unissued.  Waves 1 .. 3 leave (value, class) of their quarter in LDS (6 KB); wave 0 folds them in
// wave order with the same strict >, so the result is the first maximum over all classes, then packs the four classes into one dword.
#include "count_core.h"
#include "launchers.h"

namespace univs {

constexpr int SEMSEG_MAX_CLASSES = 256;         // a class is one byte
constexpr int CONFUSION_MAX_CELLS = 32768;      // (K + 1)^2 int32 cells = 128 KB of the 160 KB LDS of a gfx950 CU
constexpr int CONFUSION_MAX_BLOCKS = 256;       // one workgroup per CU holds the histogram; a workgroup strides over its tiles

struct __attribute__((packed, aligned(4))) Pair {                  // two neighbouring floats; the address is a multiple of 4 only
  float x, y;
};

__global__ __launch_bounds__(256) void semseg_labels_kernel(const float* __restrict__ r, int C, int hi, int wi, int H, int W, float rh,
                                                            float rw, unsigned char* __restrict__ labels) {
  __shared__ float part_v[3][64][4];
  __shared__ int part_c[3][64][4];
  const int wq = (W + 3) >> 2;                                     // groups of four per output row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long q = (long long)blockIdx.x * 64 + lane;           // (< H wq + 64 <= 2^31 + 64)
  const bool active = q < (long long)H * wq;
  const int oy = active ? (int)(q / wq) : 0, ox = active ? (int)(q - (long long)oy * wq) * 4 : 0;
  // (i0 is clamped: where a coordinate near 2^30 rounds up to in_size in fp32 -- ATen's expression has no guard -- the read stays inside
  // the plane; every index that was inside is unchanged)
  Tap ty = make_tap(rh, oy, hi);
  ty.i0 = min(ty.i0, hi - 1);
  Tap tx[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    tx[v] = make_tap(rw, min(ox + v, W - 1), wi);                  // (a column beyond the row: its neighbour's taps, not stored)
    tx[v].i0 = min(tx[v].i0, wi - 1);
  }
  const int per = (C + 3) >> 2;
  const int c0 = wave * per, c1 = min(C, c0 + per);
  const long long plane = (long long)hi * wi;
  const float* r0 = r + (long long)c0 * plane + (long long)ty.i0 * wi;
  const long long dy = (long long)ty.di * wi;
  float best[4] = {0.f, 0.f, 0.f, 0.f};
  int arg[4] = {-1, -1, -1, -1};                                    // -1: this wave has no class (C < 4)
  if (active && wi >= 2) {
    // the two taps of a row are neighbours: ONE 8-byte load per row and pixel (8 loads per class instead of 16).  In the last column
    // (di = 0) the pair starts one column earlier, so that it ends inside the row, and both taps are its second value.
    int xo[4];
    bool edge[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) xo[v] = min(tx[v].i0, wi - 2), edge[v] = tx[v].i0 > wi - 2;
#pragma unroll 2
    for (int c = c0; c < c1; ++c, r0 += plane) {
      const float* r1 = r0 + dy;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const Pair p0 = *reinterpret_cast<const Pair*>(r0 + xo[v]), p1 = *reinterpret_cast<const Pair*>(r1 + xo[v]);
        const float u = bilerp(ty, tx[v], edge[v] ? p0.y : p0.x, p0.y, edge[v] ? p1.y : p1.x, p1.y);
        if (arg[v] < 0 || u > best[v]) best[v] = u, arg[v] = c;
      }
    }
  } else if (active) {                                             // planes of one column
    for (int c = c0; c < c1; ++c, r0 += plane) {
      const float* r1 = r0 + dy;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float u = bilerp(ty, tx[v], r0[tx[v].i0], r0[tx[v].i0 + tx[v].di], r1[tx[v].i0], r1[tx[v].i0 + tx[v].di]);
        if (arg[v] < 0 || u > best[v]) best[v] = u, arg[v] = c;
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int v = 0; v < 4; ++v) part_v[wave - 1][lane][v] = best[v], part_c[wave - 1][lane][v] = arg[v];
  }
  __syncthreads();
  if (wave != 0 || !active) return;
#pragma unroll
  for (int w = 0; w < 3; ++w) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float u = part_v[w][lane][v];
      const int c = part_c[w][lane][v];
      if (c >= 0 && u > best[v]) best[v] = u, arg[v] = c;         // (wave 0 always has a class: C >= 1)
    }
  }
  unsigned char* dst = labels + (long long)oy * W + ox;
  if (ox + 3 < W && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
    *reinterpret_cast<unsigned*>(dst) = (unsigned)arg[0] | ((unsigned)arg[1] << 8) | ((unsigned)arg[2] << 16) | ((unsigned)arg[3] << 24);
  } else {                                                         // W % 4 != 0: the row's last group, and rows that start off a dword
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (ox + v < W) dst[v] = (unsigned char)arg[v];
  }
}

int semseg_labels_f32(const float* r, int C, int hi, int wi, int H, int W, unsigned char* labels, hipStream_t st) {
  if (C > SEMSEG_MAX_CLASSES || (long long)H * W >= (1LL << 31) || (long long)hi * wi >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  const float rh = (float)hi / (float)H, rw = (float)wi / (float)W;   // (as bilinear_resample_f32)
  const long long groups = (long long)H * ((W + 3) / 4);
  hipLaunchKernelGGL(semseg_labels_kernel, dim3((unsigned)((groups + 63) / 64)), dim3(256), 0, st, r, C, hi, wi, H, W, rh, rw, labels);
  return check_launch("semseg_labels_f32");
}

// ---- conf[(K + 1) row + col] += 1 per pixel, row = the ground truth (ignore_label -> K), col = the prediction ---------------------------
// A workgroup of 256 threads strides over tiles of 1024 pixels; a lane owns four consecutive pixels, one dword of each map (the maps are
// dword-aligned; the last dword of a map may reach up to three bytes past n, inside the allocation's rounding as in vss_count.hip).  The
// cells go to the LDS histogram through hist_add4 and reach the 64-bit matrix once per workgroup, non-zero cells only.  A ground-truth
// byte that is neither < K nor the ignore label, and a prediction byte > K, index nothing: they are counted in stray[0] / stray[1].
__global__ __launch_bounds__(256) void label_confusion_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                              int n, int K, int ignore_label, unsigned long long* __restrict__ conf,
                                                              unsigned long long* __restrict__ stray) {
  extern __shared__ int confusion_lds[];                           // histogram [(K + 1)^2]
  const int cells = (K + 1) * (K + 1);
  hist_zero_n(confusion_lds, cells);
  const int groups = (int)(((long long)n + 3) >> 2);
  const int tiles = (groups + 255) >> 8;
  int bad_g = 0, bad_p = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {    // (uniform over the workgroup: hist_add4's ballot sees every lane)
    const int grp = (tile << 8) + threadIdx.x;
    const int m = grp < groups ? (int)min(4LL, (long long)n - 4LL * grp) : 0;
    unsigned g4 = 0, p4 = 0;
    if (m > 0) {
      g4 = *reinterpret_cast<const unsigned*>(gt + 4LL * grp);
      p4 = *reinterpret_cast<const unsigned*>(pred + 4LL * grp);
    }
    int cell[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cell[j] = -1;
      if (j < m) {
        const int g = (int)((g4 >> (8 * j)) & 255u), p = (int)((p4 >> (8 * j)) & 255u);
        const int row = g == ignore_label ? K : (g < K ? g : -1);
        if (row < 0) ++bad_g;
        else if (p > K) ++bad_p;
        else cell[j] = (K + 1) * row + p;
      }
    }
    hist_add4(confusion_lds, cell);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += 256)
    if (confusion_lds[i]) atomicAdd(conf + i, (unsigned long long)confusion_lds[i]);
  bad_g = wave_sum(bad_g);
  bad_p = wave_sum(bad_p);
  if ((threadIdx.x & 63) == 0) {
    if (bad_g) atomicAdd(stray + 0, (unsigned long long)bad_g);
    if (bad_p) atomicAdd(stray + 1, (unsigned long long)bad_p);
  }
}

int label_confusion_u8(const unsigned char* gt, const unsigned char* pred, long long n, int K, int ignore_label, long long* conf,
                       long long* stray, hipStream_t st) {
  const long long cells = ((long long)K + 1) * ((long long)K + 1);
  if (cells > CONFUSION_MAX_CELLS || n >= (1LL << 31) - 4 || ((uintptr_t)gt & 3) || ((uintptr_t)pred & 3) || ((uintptr_t)conf & 7) ||
      ((uintptr_t)stray & 7))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  const int tiles = (int)((((n + 3) >> 2) + 255) >> 8);
  // a workgroup's share is at most ceil(tiles / blocks) * 1024 < 2^31 pixels: an int32 cell cannot wrap
  launch_lds(&label_confusion_kernel, dim3((unsigned)std::min(tiles, CONFUSION_MAX_BLOCKS)), (size_t)cells * sizeof(int), st, gt, pred, (int)n,
             K, ignore_label, reinterpret_cast<unsigned long long*>(conf), reinterpret_cast<unsigned long long*>(stray));
  return check_launch("label_confusion_u8");
}

}  // namespace univs
