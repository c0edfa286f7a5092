// The prompts of a VOS video straight from its annotation PNGs' id maps (include/univs_idmap_hip.h): which values a frame holds, how
// often and where (the census), and every listed object's mask at the model's input size with its box (the prompts).  An id map is
// uint8 [H, W], a pixel's value is its object's id.  Pillow's NEAREST resize is a pure gather, so the resized plane of value v is
// (resized id map == v): one read of a frame's bytes serves all of its objects, no per-object plane at the source size and no
// run-length code exists.  The sibling csrc/mask_prompt_resize.hip does the same from run-length codes, one workgroup per mask.
//
// Both kernels walk a frame in workgroups of 256 threads that own a segment of rows (row_segments of mask_post.h); a wave owns a quarter
// of the segment's rows and a lane FOUR adjacent columns, which it reads (census: one dword where the address is 4-byte aligned) or
// writes (prompts: one dword per plane where the address is) at once.  Down its rows a lane keeps the value it saw last with that run's
// count and extremes in registers and touches the workgroup's LDS table -- 256 counters and 256 x {xmin, ymin, xmax, ymax} -- only when
// the value changes: an id map is made of regions, so that is rare, and a lane whose four bytes all repeat the last value pays one
// comparison.  The table reaches global memory once per workgroup, one thread per value or per listed object, with atomics
// (idmap_init_kernel before sets the records to "untouched", idmap_finish_kernel after turns them into {x0, y0, x1 + 1, y1 + 1} or zeros).
//
// Prompts: a workgroup owns IM_TW = 256 output columns of its rows of one FRAME.  `frame` is non-decreasing, so the frame's objects are
// one slice [n0, n1) of the list, found by two binary searches.  Per output row a lane gathers its four source bytes once (not at all
// where ty repeats the row before) and then writes four bytes of every plane of the slice: the source is read once per frame, whatever
// the number of objects.  The extremes are kept per VALUE (of the resized map), not per listed object: a value listed twice needs no
// second slot, a listed value that is absent finds an untouched record, and an object's box is its value's record.
//
// frame, value, ty and tx are clamped before use: bad entries cost wrong pixels (a `frame` that goes down: planes that are not written),
// never an address outside the inputs.  There is no floating point here: the tables come from the caller (data/resize_rule.py).
#include <stdint.h>

#include "launchers.h"
#include "mask_post.h"

namespace univs {

constexpr int IM_TW = 256;                                         // columns of a workgroup's tile: four per lane
constexpr int IM_FRAMES_Y = 65535;                                 // frames across grid.y; a workgroup strides over the rest

// records [n][4] -> "untouched", and n_zero counters -> 0
__global__ __launch_bounds__(256) void idmap_init_kernel(int* __restrict__ box, long long n, int* __restrict__ count, long long n_zero) {
  const long long step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 4 * n; i += step) box[i] = (i & 3) < 2 ? INT_MAX : -1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_zero; i += step) count[i] = 0;
}

__global__ __launch_bounds__(256) void idmap_finish_kernel(int* __restrict__ box, long long n) {
  const long long step = (long long)gridDim.x * 256;
  for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < n; m += step) {
    int* o = box + 4 * m;
    const int xmin = o[0], ymin = o[1], xmax = o[2], ymax = o[3];
    const bool any = ymax >= 0;
    o[0] = any ? xmin : 0;
    o[1] = any ? ymin : 0;
    o[2] = any ? xmax + 1 : 0;
    o[3] = any ? ymax + 1 : 0;
  }
}

// ---- a lane's current run: the value it saw last, how often, and where --------------------------------------------------------------------
struct Run {
  int v, n, xmin, xmax, ymin, ymax;                                // v < 0: none yet
};

template <bool COUNT>
__device__ __forceinline__ void run_flush(const Run& r, int* cnt, int* ext) {
  if (r.v < 0) return;
  if constexpr (COUNT) atomicAdd(&cnt[r.v], r.n);
  atomicMin(&ext[4 * r.v + 0], r.xmin);
  atomicMin(&ext[4 * r.v + 1], r.ymin);
  atomicMax(&ext[4 * r.v + 2], r.xmax);
  atomicMax(&ext[4 * r.v + 3], r.ymax);
}

// the nb <= 4 bytes of `w` (byte j: column x + j of row y) join the run or end it
template <bool COUNT>
__device__ __forceinline__ void run_push(Run& r, unsigned w, int nb, int x, int y, int* cnt, int* ext) {
  if (nb == 4 && r.v >= 0 && w == (unsigned)r.v * 0x01010101u) {   // the common case: all four repeat the run's value
    r.n += 4;
    r.xmin = min(r.xmin, x);
    r.xmax = max(r.xmax, x + 3);
    r.ymin = min(r.ymin, y);
    r.ymax = max(r.ymax, y);
    return;
  }
  for (int j = 0; j < nb; ++j) {
    const int v = (w >> (8 * j)) & 255;
    if (v == r.v) {
      r.n += 1;
      r.xmin = min(r.xmin, x + j);
      r.xmax = max(r.xmax, x + j);
      r.ymin = min(r.ymin, y);
      r.ymax = max(r.ymax, y);
    } else {
      run_flush<COUNT>(r, cnt, ext);
      r = Run{v, 1, x + j, x + j, y, y};
    }
  }
}

__device__ __forceinline__ void table_init(int* cnt, int* ext) {   // by all 256 threads
  if (cnt) cnt[threadIdx.x] = 0;
  ext[4 * threadIdx.x + 0] = INT_MAX;
  ext[4 * threadIdx.x + 1] = INT_MAX;
  ext[4 * threadIdx.x + 2] = -1;
  ext[4 * threadIdx.x + 3] = -1;
  __syncthreads();
}

__device__ __forceinline__ void record_merge(int* __restrict__ o, const int* e) {
  atomicMin(o + 0, e[0]);
  atomicMin(o + 1, e[1]);
  atomicMax(o + 2, e[2]);
  atomicMax(o + 3, e[3]);
}

// ---- the census: grid (row segments, frames) ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void idmap_census_kernel(const unsigned char* __restrict__ ids, int F, int H, int W, int rows_per_seg,
                                                           int* __restrict__ count, int* __restrict__ box) {
  __shared__ int cnt[256];
  __shared__ int ext[256 * 4];
  const int y0 = blockIdx.x * rows_per_seg, y1 = min(H, y0 + rows_per_seg);
  if (y0 >= y1) return;                                            // (the whole workgroup: no barrier is skipped by a part of it)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows_per_wave = (y1 - y0 + 3) >> 2;
  const int ya = y0 + wave * rows_per_wave, yb = min(y1, ya + rows_per_wave);
  for (int f = blockIdx.y; f < F; f += gridDim.y) {
    table_init(cnt, ext);
    const unsigned char* plane = ids + (long long)f * H * W;       // F H W < 2^31
    Run r{-1, 0, 0, 0, 0, 0};
    for (int x = 4 * lane; x < W; x += IM_TW)                      // down the rows first: a region's run goes on
      for (int y = ya; y < yb; ++y) {
        const unsigned char* p = plane + (long long)y * W + x;
        const int nb = min(4, W - x);
        unsigned w = 0;
        if (nb == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
          w = *reinterpret_cast<const unsigned*>(p);
        } else {
          for (int j = 0; j < nb; ++j) w |= (unsigned)p[j] << (8 * j);
        }
        run_push<true>(r, w, nb, x, y, cnt, ext);
      }
    run_flush<true>(r, cnt, ext);
    __syncthreads();
    const int v = threadIdx.x;                                     // one value per thread
    if (cnt[v]) {
      atomicAdd(count + (long long)f * 256 + v, cnt[v]);
      record_merge(box + ((long long)f * 256 + v) * 4, ext + 4 * v);
    }
    __syncthreads();                                               // (the table is set again for the next frame)
  }
}

// ---- the prompts: grid (column tiles x row segments, frames) ------------------------------------------------------------------------------
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// the first n in [0, N) whose clamped frame is >= f (N: none)
__device__ __forceinline__ int first_of_frame(const int* __restrict__ frame, int N, int F, int f) {
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (clampi(frame[mid], 0, F - 1) < f) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void idmap_prompts_kernel(const unsigned char* __restrict__ ids, int F, int H, int W,
                                                            const int* __restrict__ frame, const int* __restrict__ value, int N,
                                                            const int* __restrict__ ty, const int* __restrict__ tx, int Ho, int Wo,
                                                            int tiles_x, int rows_per_seg, unsigned char* __restrict__ masks,
                                                            int* __restrict__ boxes) {
  __shared__ int ext[256 * 4];
  const int tile = blockIdx.x % tiles_x, seg = blockIdx.x / tiles_x;
  const int y0 = seg * rows_per_seg, y1 = min(Ho, y0 + rows_per_seg);
  if (y0 >= y1) return;                                            // (the whole workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows_per_wave = (y1 - y0 + 3) >> 2;
  const int ya = y0 + wave * rows_per_wave, yb = min(y1, ya + rows_per_wave);
  const int xo = tile * IM_TW + 4 * lane;
  const int nb = min(4, Wo - xo);                                  // <= 0: the lane has no column
  int sx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sx[j] = clampi(tx[min(xo + j, Wo - 1)], 0, W - 1);

  for (int f = blockIdx.y; f < F; f += gridDim.y) {
    const int n0 = first_of_frame(frame, N, F, f), n1 = f + 1 < F ? first_of_frame(frame, N, F, f + 1) : N;
    if (n0 >= n1) continue;                                        // (uniform: the frame lists no object)
    table_init(nullptr, ext);
    Run r{-1, 0, 0, 0, 0, 0};
    int prev = -1;
    unsigned w = 0;
    if (nb > 0) {
      for (int yo = ya; yo < yb; ++yo) {
        const int sy = clampi(ty[yo], 0, H - 1);
        if (sy != prev) {                                          // (an up-scale repeats source rows)
          const unsigned char* row = ids + ((long long)f * H + sy) * W;
          w = (unsigned)row[sx[0]] | (unsigned)row[sx[1]] << 8 | (unsigned)row[sx[2]] << 16 | (unsigned)row[sx[3]] << 24;
          prev = sy;
        }
        run_push<false>(r, w, nb, xo, yo, nullptr, ext);
        for (int n = n0; n < n1; ++n) {
          const unsigned v = (unsigned)clampi(value[n], 0, 255);
          const unsigned m = (unsigned)((w & 255u) == v) | (unsigned)(((w >> 8) & 255u) == v) << 8 |
                             (unsigned)(((w >> 16) & 255u) == v) << 16 | (unsigned)((w >> 24) == v) << 24;
          unsigned char* d = masks + ((long long)n * Ho + yo) * Wo + xo;   // N Ho Wo < 2^31
          if (nb == 4 && (reinterpret_cast<uintptr_t>(d) & 3) == 0) {
            *reinterpret_cast<unsigned*>(d) = m;
          } else {
            for (int j = 0; j < nb; ++j) d[j] = (unsigned char)((m >> (8 * j)) & 1u);
          }
        }
      }
    }
    run_flush<false>(r, nullptr, ext);
    __syncthreads();
    for (int n = n0 + (int)threadIdx.x; n < n1; n += 256) {        // an object's box is its value's record
      const int v = clampi(value[n], 0, 255);
      if (ext[4 * v + 3] >= 0) record_merge(boxes + 4LL * n, ext + 4 * v);
    }
    __syncthreads();                                               // (the table is set again for the next frame)
  }
}

int idmap_census_u8(const unsigned char* ids, int F, int H, int W, int* count, int* box, hipStream_t st) {
  if ((long long)F * H * W >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  const int fy = std::min(F, IM_FRAMES_Y);
  int rows_per_seg = 0;
  const int segs = row_segments(H, fy, &rows_per_seg);
  const long long records = 256LL * F;
  hipLaunchKernelGGL(idmap_init_kernel, dim3(flat_blocks(4 * records, 2048)), dim3(256), 0, st, box, records, count, records);
  hipLaunchKernelGGL(idmap_census_kernel, dim3((unsigned)segs, (unsigned)fy), dim3(256), 0, st, ids, F, H, W, rows_per_seg, count, box);
  hipLaunchKernelGGL(idmap_finish_kernel, dim3(flat_blocks(records, 2048)), dim3(256), 0, st, box, records);
  return check_launch("idmap_census_u8");
}

int idmap_prompts_u8(const unsigned char* ids, int F, int H, int W, const int* frame, const int* value, int N, const int* ty, const int* tx,
                     int Ho, int Wo, unsigned char* masks, int* boxes, hipStream_t st) {
  if ((long long)F * H * W >= (1LL << 31) || (long long)N * Ho * Wo >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  const long long tiles_x = (Wo + IM_TW - 1) / IM_TW;
  const int fy = std::min(std::min(F, N), IM_FRAMES_Y);            // (no more frames than objects hold an object)
  int rows_per_seg = 0;
  const long long segs = row_segments(Ho, tiles_x * fy, &rows_per_seg);
  hipLaunchKernelGGL(idmap_init_kernel, dim3(flat_blocks(4LL * N, 2048)), dim3(256), 0, st, boxes, (long long)N, (int*)nullptr, 0LL);
  hipLaunchKernelGGL(idmap_prompts_kernel, dim3((unsigned)(tiles_x * segs), (unsigned)std::min(F, IM_FRAMES_Y)), dim3(256), 0, st, ids, F, H, W,
                     frame, value, N, ty, tx, Ho, Wo, (int)tiles_x, rows_per_seg, masks, boxes);   // tiles_x segs <= Ho Wo < 2^31
  hipLaunchKernelGGL(idmap_finish_kernel, dim3(flat_blocks(N, 2048)), dim3(256), 0, st, boxes, (long long)N);
  return check_launch("idmap_prompts_u8");
}

}  // namespace univs
