// What the count kernels of the evaluation share (pair_count.hip, vss_count.hip, davis_count.hip): from mask_post.h the wave reductions,
// the LDS histogram of n cells (hist_zero_n / hist_flush_n) and row_segments; here the step that adds a lane's four cells to that
// histogram, the one reduction mask_post.h has no use for, and the launch with dynamic LDS beyond 64 KB.
#pragma once
#include "mask_post.h"

namespace univs {

__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v |= (unsigned)__shfl_xor((int)v, m, 64);
  return v;
}

// hist[cell[j]] += 1 for the lane's four consecutive pixels; a cell < 0 is "no pixel".  EVERY lane of the wave calls it, a lane without
// pixels with four cells < 0: the caller's trip count is uniform over the wave, because the ballot has to see all 64 lanes.  When the
// whole wave holds one cell, one lane adds 256; otherwise a lane adds each of its runs of equal cells with one LDS atomic.
// (cell[4] comes as a pointer on purpose: behind a reference to int[4] the compiler makes the three comparisons branchless before it
// inlines this into the kernels, whose instruction streams then differ from the ones that were measured.)
__device__ __forceinline__ void hist_add4(int* hist, const int* cell) {
  const bool one = cell[0] == cell[1] && cell[1] == cell[2] && cell[2] == cell[3];
  const int lead = __builtin_amdgcn_readfirstlane(cell[0]);
  if (__ballot(one && cell[0] == lead) == ~0ull) {
    if ((threadIdx.x & 63) == 0 && lead >= 0) atomicAdd(&hist[lead], 256);
  } else {
    int run = 1;
#pragma unroll
    for (int j = 1; j <= 4; ++j) {
      if (j < 4 && cell[j] == cell[j - 1]) {
        ++run;
      } else {
        if (cell[j - 1] >= 0) atomicAdd(&hist[cell[j - 1]], run);
        run = 1;
      }
    }
  }
}

// `k` over `grid` workgroups of 256 threads with `lds` bytes of dynamic LDS on `st`; beyond the 64 KB a kernel may take by default the
// function's limit is raised first.  The caller checks the launch under its own name (check_launch).
template <typename... Params, typename... Args>
inline void launch_lds(void (*k)(Params...), dim3 grid, size_t lds, hipStream_t st, Args... args) {
  if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(k, grid, dim3(256), lds, st, args...);
}

}  // namespace univs
