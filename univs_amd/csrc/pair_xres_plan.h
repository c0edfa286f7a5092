// What linear_pair_xres.hip covers of the calls of univs_encoder_linear_pair_presplit_f32, decided on the host and free of HIP
// (tools/encoder_xres_plan.cpp prints it, tests/test_encoder_pair_xres_cpu.py compares it with the entry's documented rules).
// The ENTRY's coverage does not change: a call is answered as before (pair_covered and the one instantiation of linear_pair_f16x3,
// gemm_plan.h); inside that set the x-resident kernel takes the calls whose feature counts are whole 32-feature chunks.
#pragma once
#include "gemm_plan.h"

namespace univs {

constexpr int PX_THREADS = 512;   // 8 waves, two per SIMD: one workgroup per CU
constexpr int PX_ROWS = 128;      // rows of a group: 16 per wave
constexpr int PX_CHUNK = 32;      // features of a W chunk (two MFMA feature blocks)
constexpr int PX_IMAGES = 4;      // chunk images in LDS: the current chunk, the two after it, and the one being requested

// bytes of LDS: PX_IMAGES chunk images [(K / 8) x 2 parts][32 features] of 16-byte units | bias and inverse scales of both problems
inline size_t pair_xres_lds(int N_a, int N_b, int K) { return (size_t)PX_IMAGES * (K / 8) * 2 * PX_CHUNK * 16 + (size_t)2 * (N_a + N_b) * 4; }

inline bool pair_xres_covered(long long M, int N_a, int N_b, int K, long long add_rows, long long blk_rows, int blk_cols_a, int blk_cols_b,
                              int n_cu) {
  if (!pair_covered(M, N_a, N_b, K, add_rows, blk_rows, blk_cols_a, blk_cols_b)) return false;
  const PairPlan p = plan_f16x3_pair(M, N_a, N_b, K, n_cu);
  if (!p.covered || p.RB[0] != 8 || p.RB[1] != 6 || p.ring != 4) return false;   // what the entry answers at all
  // the one instantiation: 8 k-steps; whole chunks, and at least as many per problem as the stream runs ahead
  constexpr int N_MIN = (PX_IMAGES - 1) * PX_CHUNK;
  if (K != 256 || N_a % PX_CHUNK != 0 || N_b % PX_CHUNK != 0 || N_a < N_MIN || N_b < N_MIN) return false;
  return pair_xres_lds(N_a, N_b, K) <= (size_t)RESIDENT_LDS_CAP;
}
// workgroups: persistent over the row groups, one per CU
inline unsigned pair_xres_grid(long long M, int n_cu) { return (unsigned)std::min<long long>(n_cu, (M + PX_ROWS - 1) / PX_ROWS); }

// linear_pair_xres.hip: returns 1 if launched, 0 if not covered (or switched off), < 0 on error.  `stream`: a hipStream_t
int linear_pair_xres_f32(const float* x, const float* add, long long add_rows, const void* wp_a, const float* winv_a, const float* bias_a,
                         int N_a, int blk_cols_a, float* y_a, const void* wp_b, const float* winv_b, const float* bias_b, int N_b,
                         int blk_cols_b, float* y_b, long long M, int K, long long blk_rows, void* stream);

}  // namespace univs
