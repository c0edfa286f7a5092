// Everything the VSPW scores need from one video, in one pass: the confusion matrix of mIoU and the per-window pixel counts of the video
// consistency scores VC8 / VC16 (univs_amd/evaluation/vss.py).  The reference compares, for every window start i, frame i with each of
// the next 7 (then 15) frames on both sides over full-size float planes, after a pass of its own for the confusion matrix
// (univs/evaluation/vss_evaluation.py:130-224, :235-251, eval_utils_vss.py:96-105): every pixel is read about 50 times.
//
// gt / pred: uint8 [T, H, W], the raw VSPW mask values and the bytes of the prediction PNGs.  The ground truth goes through
// `map_category_id` here (vss_evaluation.py:226-232: 0 -> 255, v -> v - 1, 254 -> 255, in uint8, so raw 255 ends as 255 too); every
// comparison below is on mapped values.
//
//   confusion [C, C]   cell C g + p += 1 for a pixel with mapped gt g < C and prediction byte p (not clamped: p >= C lands in a later
//                      row, as np.bincount(...).reshape does it).  A cell >= C C is not counted; overflow[0] = the largest such cell.
//   windows [T, 2, 2]  [i][n in {8, 16}][den, num]: the pixels whose mapped gt is equal over frames i .. i + n - 1, and those where the
//                      prediction is too (`get_common`).  "Equal to frame i over the window" is "unchanged from frame to frame", so a
//                      pixel carries two run lengths, saturating at 16: gt unchanged for r frames, gt and pred both unchanged for r
//                      frames.  The window of length n that ends at frame t is common iff the run is >= n.
//
// A workgroup of 256 threads strides over tiles of 1024 pixel positions and walks the T frames of each; a lane owns four consecutive
// pixels: one dword of each map per frame (two when the frame's base is not dword-aligned: H W need not be a multiple of 4), never a
// byte load, and the next frame's dwords are in flight while this one is counted.  The window counts are summed over the wave before
// one lane adds them in LDS; the confusion cells go to the LDS histogram through count_core.h's hist_add4 (one atomic per wave that holds
// one cell, else one per run of a lane's four pixels).  Both reach global memory once per workgroup.
//
// LDS: C C <= 16384 cells = 64 KB (the bound of pair_count.hip's PAIR_MAX_CELLS) + T <= 1024 window records of 4 ints = 16 KB: 80 KB,
// so two workgroups fit the 160 KB of a gfx950 CU (arithmetic, not a measured occupancy).
#include "count_core.h"
#include "launchers.h"

namespace univs {

constexpr int VSS_MAX_CELLS = 16384;   // C C
constexpr int VSS_MAX_FRAMES = 1024;   // T: the window records in LDS
constexpr int VSS_MAX_BLOCKS = 1024;   // ~4 per CU; a workgroup strides over its tiles

// the four bytes at byte offset `o` of a dword-aligned buffer whose end, rounded up to a dword, is `end` bytes in: no load starts at or
// beyond `end`.  The bytes the caller uses lie inside the buffer, so the second dword exists whenever one of them is in it.
__device__ __forceinline__ unsigned load_bytes4(const unsigned char* __restrict__ base, int end, int o) {
  const int a = o & 3, w0 = o - a;
  const unsigned lo = *reinterpret_cast<const unsigned*>(base + w0);
  if (a == 0) return lo;
  const unsigned hi = w0 + 4 < end ? *reinterpret_cast<const unsigned*>(base + w0 + 4) : 0u;
  return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (8 * a));
}

// map_category_id on one byte
__device__ __forceinline__ int map_gt(unsigned raw) {
  const unsigned m = (raw - 1u) & 255u;
  return m == 254u ? 255 : (int)m;
}

__global__ __launch_bounds__(256) void vss_count_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                        int end, int T, int HW, int C, int* __restrict__ confusion,
                                                        int* __restrict__ windows, int* __restrict__ overflow) {
  extern __shared__ int vss_lds[];                                // histogram [C C], window records [T][4]
  const int cells = C * C;
  int* hist = vss_lds;
  int* win = vss_lds + cells;
  hist_zero_n(vss_lds, cells + 4 * T);

  const int groups = (HW + 3) >> 2;
  const int tiles = (groups + 255) >> 8;
  int over = -1;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform over the workgroup: the ballot and the sums see every lane)
    const int grp = (tile << 8) + threadIdx.x;
    const int n = grp < groups ? min(4, HW - 4 * grp) : 0;
    int pg[4], pp[4], rg[4], rb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) pg[j] = pp[j] = -1, rg[j] = rb[j] = 0;
    unsigned gw = 0, pw = 0;
    if (n > 0) {
      gw = load_bytes4(gt, end, 4 * grp);
      pw = load_bytes4(pred, end, 4 * grp);
    }
    for (int t = 0; t < T; ++t) {
      const unsigned g4 = gw, p4 = pw;
      if (n > 0 && t + 1 < T) {                                   // the next frame, in flight during this one
        const int o = (t + 1) * HW + 4 * grp;                     // (< T H W < 2^31)
        gw = load_bytes4(gt, end, o);
        pw = load_bytes4(pred, end, o);
      }
      int cell[4], c8 = 0, c16 = 0;                               // c8 / c16: den in the low half, num in the high half
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cell[j] = -1;
        if (j < n) {
          const int g = map_gt((g4 >> (8 * j)) & 255u), p = (int)((p4 >> (8 * j)) & 255u);
          const bool same_g = g == pg[j], same_b = same_g && p == pp[j];
          rg[j] = same_g ? min(rg[j] + 1, 16) : 1;
          rb[j] = same_b ? min(rb[j] + 1, 16) : 1;
          pg[j] = g;
          pp[j] = p;
          c8 += (rg[j] >= 8 ? 1 : 0) + (rb[j] >= 8 ? 0x10000 : 0);
          c16 += (rg[j] >= 16 ? 1 : 0) + (rb[j] >= 16 ? 0x10000 : 0);
          if (g < C) {
            const int c = C * g + p;
            if (c < cells) cell[j] = c;
            else over = max(over, c);
          }
        }
      }
      // the windows that end at this frame (a wave's sum is at most 256 per half)
      if (t >= 7) {
        c8 = wave_sum(c8);
        if ((threadIdx.x & 63) == 0 && c8) {
          atomicAdd(&win[4 * (t - 7) + 0], c8 & 0xFFFF);
          if (c8 >> 16) atomicAdd(&win[4 * (t - 7) + 1], c8 >> 16);
        }
      }
      if (t >= 15) {
        c16 = wave_sum(c16);
        if ((threadIdx.x & 63) == 0 && c16) {
          atomicAdd(&win[4 * (t - 15) + 2], c16 & 0xFFFF);
          if (c16 >> 16) atomicAdd(&win[4 * (t - 15) + 3], c16 >> 16);
        }
      }
      hist_add4(hist, cell);
    }
  }
  hist_flush_n(hist, cells, confusion);
  for (int i = threadIdx.x; i < 4 * T; i += 256)                  // (behind hist_flush_n's barrier)
    if (win[i]) atomicAdd(windows + i, win[i]);
  over = wave_max(over);
  if ((threadIdx.x & 63) == 0 && over >= 0) atomicMax(overflow, over);
}

int vss_video_counts(const unsigned char* gt, const unsigned char* pred, int T, int H, int W, int C, int* confusion, int* windows,
                     int* overflow, hipStream_t st) {
  const long long hw = (long long)H * W;                          // (< 2^62; T <= 1024 below keeps the product in range)
  if ((long long)C * C > VSS_MAX_CELLS || T > VSS_MAX_FRAMES || hw >= (1LL << 31) || hw * T >= (1LL << 31) - 4 || ((uintptr_t)gt & 3) ||
      ((uintptr_t)pred & 3))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  const long long px = hw * T;
  const int HW = H * W;
  const int end = (int)((px + 3) & ~3LL);
  const int tiles = ((HW + 3) / 4 + 255) / 256;
  const size_t lds = ((size_t)C * C + 4 * (size_t)T) * sizeof(int);
  launch_lds(&vss_count_kernel, dim3((unsigned)std::min(tiles, VSS_MAX_BLOCKS)), lds, st, gt, pred, end, T, HW, C, confusion, windows, overflow);
  return check_launch("vss_video_counts");
}

}  // namespace univs
