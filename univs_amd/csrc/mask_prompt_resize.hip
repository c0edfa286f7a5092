// The first-frame masks of a VOS video at the model's input size (include/univs_prompts_hip.h): Pillow's NEAREST resize of every
// annotated mask and the box of the result, straight from the run-length codes.  The reference does this per object on a host core
// (dataset_mapper_uni_vid.py:456-486: decode a full-resolution plane, `PIL.Image.resize(NEAREST)`, stack, scan the stack for boxes);
// here no source-resolution plane exists.
//
// A mask is its cumulative column-major run boundaries (the `Runs` layout of univs_amd/evaluation/vis_counts.py): run k covers the
// pixels [b_{k-1}, b_k) of the flattened column-major plane, b_{-1} = 0, odd runs are foreground.  Output pixel (yo, xo) reads source
// pixel p = tx[xo] H + ty[yo], and its value is the parity of the number of boundaries <= p.  The two index tables are arguments
// (univs_amd/data/resize_rule.py: `nearest_table`, Pillow's running float64 sum computed on the host): there is no floating point here.
//
// A workgroup of 256 threads owns MP_TW = 64 output columns of a segment of rows of one mask.  A lane owns one column, a wave a
// quarter of the segment's rows: it finds the first boundary beyond its first pixel by one binary search and then walks down its rows,
// advancing its run pointer while bounds[k] <= p -- ty is non-decreasing, so the pointer never goes back.  The 64 lanes of a wave store
// 64 neighbouring bytes of one output row.  Neighbouring lanes read neighbouring source columns, so their boundaries share cache lines;
// the boundaries are read from global memory (L1 / L2), not staged in LDS: a mask has a few hundred to a few thousand of them and a
// workgroup reads the slice of its 64 columns once.  Nothing about this kernel's speed is claimed here; tools/prompt_masks_bench.py
// measures it.
//
// Table entries are clamped to the source before use, the mask's slice of `bounds` to [0, n_bounds], and a pointer never passes its
// slice's end: a bad table or bad starts cost wrong pixels (a pointer that would have to go back stays), never an address outside the
// inputs.  Boxes: the lanes' extremes meet through flush_record (mask_post.h: wave reductions, one set of atomics per workgroup) in
// boxes[m] = {xmin, ymin, xmax, ymax}, which box_init_kernel sets to "untouched" before and box_finish_kernel turns into
// {x0, y0, x1 + 1, y1 + 1}, or zeros for an empty or absent mask, after.
#include <stdint.h>

#include "launchers.h"
#include "mask_post.h"

namespace univs {

constexpr int MP_TW = 64;                                          // output columns of a workgroup: one per lane

__global__ __launch_bounds__(256) void box_init_kernel(int* __restrict__ boxes, int N) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < 4LL * N) boxes[i] = (i & 3) < 2 ? INT_MAX : -1;
}

__global__ __launch_bounds__(256) void box_finish_kernel(int* __restrict__ boxes, int N) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  if (m >= N) return;
  int* o = boxes + 4 * m;
  const int xmin = o[0], ymin = o[1], xmax = o[2], ymax = o[3];
  const bool any = ymax >= 0;
  o[0] = any ? xmin : 0;
  o[1] = any ? ymin : 0;
  o[2] = any ? xmax + 1 : 0;
  o[3] = any ? ymax + 1 : 0;
}

__global__ __launch_bounds__(256) void rle_mask_resize_kernel(const int* __restrict__ bounds, const int* __restrict__ starts, int n_bounds,
                                                              int H, int W, const int* __restrict__ ty, const int* __restrict__ tx, int Ho,
                                                              int Wo, int tiles_x, int segs, int rows_per_seg,
                                                              unsigned char* __restrict__ masks, int* __restrict__ boxes) {
  int blk = blockIdx.x;
  const int tile = blk % tiles_x;
  blk /= tiles_x;
  const int seg = blk % segs, m = blk / segs;
  const int y0 = seg * rows_per_seg, y1 = min(Ho, y0 + rows_per_seg);
  if (y0 >= y1) return;                                            // (the whole workgroup: no barrier is skipped by a part of it)

  // the mask's boundaries, inside `bounds` whatever `starts` holds
  const int s0 = min(max(starts[m], 0), n_bounds), s1 = min(max(starts[m + 1], s0), n_bounds);
  const int* b = bounds + s0;
  const int n = s1 - s0;                                           // 0: the mask is absent, its plane is zero

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int xo = tile * MP_TW + lane;
  const bool live = xo < Wo;
  const int base = min(max(tx[min(xo, Wo - 1)], 0), W - 1) * H;    // H W < 2^31
  const int rows_per_wave = (y1 - y0 + 3) >> 2;
  const int ya = y0 + wave * rows_per_wave, yb = min(y1, ya + rows_per_wave);
  unsigned char* dst = masks + ((size_t)m * Ho) * Wo + xo;

  int xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1;
  if (live && ya < yb) {
    // k = the number of boundaries <= p: the run that holds p
    int p = base + min(max(ty[ya], 0), H - 1);
    int k = 0, hi = n;
    while (k < hi) {
      const int mid = (k + hi) >> 1;
      if (b[mid] <= p) k = mid + 1; else hi = mid;
    }
    for (int yo = ya; yo < yb; ++yo) {
      p = base + min(max(ty[yo], 0), H - 1);
      while (k < n && b[k] <= p) ++k;
      const int v = k & 1;
      dst[(size_t)yo * Wo] = (unsigned char)v;
      if (v) {
        ymin = min(ymin, yo);
        ymax = yo;                                                 // (yo only grows)
      }
    }
    if (ymax >= 0) xmin = xmax = xo;
  }
  flush_record<false, true>(boxes + (4LL * m - 2), 0, 0, xmin, ymin, xmax, ymax);   // (-2: the record's corners sit at o[2:6])
}

int resize_rle_masks_u8(const int* bounds, const int* starts, long long n_bounds, int N, int H, int W, const int* ty, const int* tx, int Ho,
                        int Wo, unsigned char* masks, int* boxes, hipStream_t st) {
  const long long tiles_x = (Wo + MP_TW - 1) / MP_TW;
  if ((long long)H * W >= (1LL << 31) || n_bounds >= (1LL << 31) || (long long)N * Ho * Wo >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  int rows_per_seg = 0;
  const long long segs = row_segments(Ho, (long long)N * tiles_x, &rows_per_seg);
  const long long blocks = tiles_x * segs * N;                     // <= N Ho Wo < 2^31
  hipLaunchKernelGGL(box_init_kernel, dim3((unsigned)((4LL * N + 255) / 256)), dim3(256), 0, st, boxes, N);
  hipLaunchKernelGGL(rle_mask_resize_kernel, dim3((unsigned)blocks), dim3(256), 0, st, bounds, starts, (int)n_bounds, H, W, ty, tx, Ho, Wo,
                     (int)tiles_x, (int)segs, rows_per_seg, masks, boxes);
  hipLaunchKernelGGL(box_finish_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, boxes, N);
  return check_launch("resize_rle_masks_u8");
}

}  // namespace univs
