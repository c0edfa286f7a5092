// What conv3x3_wide.hip covers of the calls of conv3x3_f16x3_f32 / conv3x3_nhwc_f16x3_f32, and how it deals the rows to its workgroups:
// decided on the host and free of HIP (tools/conv3x3_wide_plan.cpp prints it, tests/test_conv3x3_wide_cpu.py compares it with the rules
// restated in Python).  The launchers' coverage does not change: inside the set stream_conv_covered answers, the wide kernel takes the
// calls with exactly 256 output features; every other call keeps the streamed kernel (gemm_f16x3_stream.hip).
#pragma once
#include "gemm_plan.h"

namespace univs {

constexpr int CW_THREADS = 512;    // 8 waves, two per SIMD: one workgroup per CU
constexpr int CW_TILE_M = 32;      // pixels of a wave tile (two 16-column MFMA tiles), as GS_TILE_M
constexpr int CW_COUT = 256;       // output features of the one instantiation: 16 MFMA feature blocks per wave
constexpr int CW_IMAGES = 4;       // k-step images of W in LDS: the current pair of k-steps and the pair being requested

// a k-step's image: [4 k-groups][2 parts][256 features] 16-byte units = the contiguous 32 KB of the pre-split image of presplit_f16x3
constexpr size_t CW_IMAGE_BYTES = (size_t)4 * 2 * CW_COUT * 16;
// bytes of LDS: CW_IMAGES images | bias[256] | winv[256]
inline size_t conv3x3_wide_lds() { return CW_IMAGES * CW_IMAGE_BYTES + (size_t)2 * CW_COUT * 4; }

// Covered: what the streamed kernel covers of a 3 x 3 (Cin % 128 == 0, Cout % 16 == 0, M >= 4096, byte offsets below 2^31) with
// Cout == 256.  (Cin % 128 == 0: an even number of k-steps per tap -- the register ring of x holds two.)
inline bool conv3x3_wide_covered(long long M, int Cin, int Cout) {
  return stream_conv_covered(M, Cin, Cout, 9) && Cout == CW_COUT && conv3x3_wide_lds() <= (size_t)RESIDENT_LDS_CAP;
}

// Row ranges.  A round of a workgroup is 8 wave tiles (256 pixels) through all 9 Cin / 32 k-steps, and the launch lasts as long as its
// workgroup with the most rounds: `rounds` = the fewest that n_cu workgroups need, `nwg` = the fewest workgroups that cover the rows
// with that many -- so no workgroup's last round is idle (294 400 pixels on 256 CUs: 1 150 rounds = 230 workgroups x 5, where one
// workgroup per CU would run 5 rounds on some and 4 on others for the same time).  Workgroup b runs rounds b * rounds .. of the
// sequence: wave tile (b * rounds + rd) * 8 + wave in round rd; tiles past the last one compute on the last row and store nothing.
struct WidePlan {
  unsigned nwg;
  int rounds;
};
inline WidePlan plan_conv3x3_wide(long long M, int n_cu) {
  constexpr int NWV = CW_THREADS / 64;
  const long long WT = (M + CW_TILE_M - 1) / CW_TILE_M;
  const long long total = (WT + NWV - 1) / NWV;                  // rounds in all
  WidePlan p;
  p.rounds = (int)((total + std::max(1, n_cu) - 1) / std::max(1, n_cu));
  p.nwg = (unsigned)((total + p.rounds - 1) / p.rounds);
  return p;
}

}  // namespace univs
