// What the three-product GEMM family launches, decided on the host and free of HIP: the coverage rules, the pass / row-range
// arithmetic and one plan function per kernel (linear_split.hip, linear_f16x3.hip, gemm_f16x3_stream.hip, gemm_f16x3_tile.hip).
// Everything here is a pure function of the shape, the CU count and the settings, so the host compiler alone builds it:
// tools/gemm_plan_dump.cpp prints the plans of the model's shapes and the edges, tests/test_gemm_plan_cpu.py compares them
// with the recorded table.  A launcher is: predicates -> plan -> switch over the plan's selectors -> launch.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/univs_hip.h"

namespace univs {

// ---- tile constants (the kernels include this header for them)
constexpr int LS_THREADS = 512;   // linear_bf16x6: 8 waves, two per SIMD
constexpr int LS_TILE_M = 32;     // rows of x per wave tile (two 16-column MFMA tiles)
constexpr int LS_MAX_RB = 7;
constexpr int L3_THREADS = 512;   // linear_f16x3: 8 waves, two per SIMD
constexpr int L3_TILE_M = 32;     // rows of x per wave tile (two 16-column MFMA tiles)
constexpr int L3_MAX_RB = 8;
constexpr int L3_WPT = 24;        // PRE: 16-byte units of the W slab per thread (plan_f16x3_resident checks that the slab fits)
#ifndef UNIVS_GS_THREADS
#define UNIVS_GS_THREADS 512     // (256: timing experiment `--ablate gs256` -- two 4-wave workgroups per CU where their W buffers fit)
#endif
constexpr int GS_THREADS = UNIVS_GS_THREADS;
constexpr int GS_TILE_M = 32;
constexpr int GT_THREADS = 512;
// UnivsConfig.linear_ablate: the family's timing experiments and A / B switches (include/univs_hip.h describes each value)
enum LinearAblate {
  LA_NONE = 0,
  LA_SCALE_FROZEN = 1,                                            // linear_f16x3: no running row scale
  LA_MLP_NOMFMA = 2, LA_MLP_NOREADS = 3, LA_MLP_NOACT = 4,        // mlp_f16x3<.., ABL = value - 1, ..>: results WRONG
  LA_NO_XCD_REMAP = 5,                                            // linear_f16x3 / gemm_f16x3_stream in plain block order
  LA_NO_TILE = 6,                                                 // univs_linear_presplit_f32 keeps gemm_f16x3_stream
  LA_TILE_NSLOT2 = 7, LA_TILE_NSLOT3 = 8, LA_TILE_NSLOT4 = 9,     // gemm_f16x3_tile with value - 5 k-steps of loads in flight
  LA_MLP_PHASE_SHIFT = 10,                                        // mlp_f16x3_ps
  LA_NO_PAIR_XRES = 11,                                           // the encoder pair entry keeps linear_pair_f16x3
  LA_NO_CONV_WIDE = 12,                                           // the 3 x 3 convolutions keep gemm_f16x3_stream
};
enum { EPI_NONE = 0, EPI_RELU = 1, EPI_GELU = 2, EPI_RESIDUAL = 3, EPI_BLOCKED = 4 };   // the kernels' LS_ / L3_ / GS_ / GT_EPI_* alias these

// ---- coverage predicates
// register stages of x = k-steps per group of the W stream: a divisor of K / 32 (0: K is not covered)
inline int k_ring(int K) { return K % 128 == 0 ? 4 : K % 96 == 0 ? 3 : 0; }
// the byte offsets of an [a, b] fp32 tensor fit the 31 bits of a buffer descriptor's extent
inline bool fits_int32(long long a, long long b) { return a * b * 4 < 0x7FFFFFFFLL; }
// every pointer (null included) on a 16-byte boundary
template <class... P>
inline bool aligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0; }
// the residual epilogue and the residual pointer come together
inline bool epi_consistent(int epi, int epi_max, bool has_residual) {
  return epi >= 0 && epi <= epi_max && (epi == EPI_RESIDUAL) == has_residual;
}
// EPI_BLOCKED: whole column blocks of whole 16-byte stores, whole batch elements
inline bool blocked_ok(long long M, int N, int blk_rows, int blk_cols) {
  return blk_rows >= 1 && blk_cols >= 4 && blk_cols % 4 == 0 && N % blk_cols == 0 && M % blk_rows == 0;
}

// ---- passes over N: as few as the per-pass cap allows, balanced, `rows` features each (rounded up to `round`: 4 = one
// 16-byte store, 16 = one MFMA feature block), RB feature blocks
struct PassPlan {
  int passes, rows, RB;
};
inline PassPlan plan_passes(int N, int r_cap, int round) {
  PassPlan p;
  p.passes = (N + r_cap - 1) / r_cap;
  p.rows = (N + p.passes - 1) / p.passes;
  p.rows = (p.rows + round - 1) / round * round;
  p.RB = (p.rows + 15) / 16;
  return p;
}

// ---- row ranges (the grid's x extent): one workgroup per CU over (row ranges x passes), every wave of a workgroup with at
// least `tiles_per_wave` of the WT row tiles.  Workgroups are dealt to the 8 XCDs round-robin by linear id, so an x extent
// that is a multiple of 8 puts the passes of one row range -- which stream the same rows of x -- on one XCD, where all but
// the first read of x hit L2.  Rounding down to a multiple of 8 is skipped where it would idle more than a tenth of the CUs
// (17 passes -> 15 row ranges, not 8: x then comes from the memory-side cache).  `grid_x` > 0: UnivsConfig.linear_grid_x.
inline long long plan_row_ranges(int n_cu, int passes, long long WT, int waves, int tiles_per_wave, int grid_x) {
  long long gx = std::max<long long>(1, n_cu / passes);
  gx = std::min(gx, std::max<long long>(1, WT / (tiles_per_wave * waves)));
  if (gx >= 8 && (gx - gx % 8) * 10 >= gx * 9) gx -= gx % 8;
  if (grid_x > 0) gx = std::min<long long>(grid_x, WT);
  return gx;
}

// ---- the W-resident kernels (linear_split.hip, linear_f16x3.hip)
// what univs_linear_fused_f32 / _blocked_f32 and their pre-split siblings cover, whichever arithmetic runs
inline bool resident_covered(long long M, int N, int K, int epi, int blk_rows, int blk_cols) {
  if (epi == EPI_BLOCKED && (K != 256 || !blocked_ok(M, N, blk_rows, blk_cols))) return false;
  if (K < 96 || k_ring(K) == 0 || N % 4 != 0) return false;
  if (!fits_int32(M, N) || !fits_int32(M, K)) return false;
  // K >= 768: the weights are split once per tensor and streamed (gemm_f16x3_stream.hip: univs_linear_presplit_f32); the
  // resident kernels stage W in every workgroup and only pay while the whole K of a useful number of features fits LDS
  if (K > 768) return false;
  return (M + LS_TILE_M - 1) / LS_TILE_M >= 64;            // too few rows to amortise the staging of W
}
// which arithmetic the resident entry runs: six bf16 products only where asked for and W is raw (the pre-split image is fp16 parts)
inline bool resident_six_products(const UnivsConfig& cfg, bool presplit) { return cfg.linear_terms == 6 && !presplit; }
struct ResidentPlan {
  bool covered;
  int RB, ksc, ring;             // linear_bf16x6<RB, ksc, ring, epi> / linear_f16x3<RB, ring, PRE>
  unsigned gx, passes;           // grid
  size_t lds;
  int rows_per_pass;
};
constexpr long long RESIDENT_LDS_CAP = 160 * 1024 - 2048;   // W slab + bias (+ inverse scales, row maxima) + the zeroed tail
inline ResidentPlan plan_bf16x6_resident(long long M, int N, int K, int epi, int n_cu) {
  ResidentPlan p{};
  int r_cap = (int)std::min<long long>(RESIDENT_LDS_CAP / ((long long)K * 6), 16 * LS_MAX_RB);
  r_cap -= r_cap % 4;
  if (r_cap < 16) return p;
  const PassPlan pp = plan_passes(N, r_cap, 4);
  const long long WT = (M + LS_TILE_M - 1) / LS_TILE_M;
  p.covered = true;
  p.RB = pp.RB;
  // a straight-line tile body for K = 256 (MSDeformAttn), a runtime k loop for anything else (straight-line bodies for
  // the Swin widths 96 .. 768 were measured: no gain, 80 s of compile time)
  p.ksc = (epi == EPI_BLOCKED || K == 256) ? 8 : 0;
  p.ring = p.ksc ? 4 : k_ring(K);
  p.gx = (unsigned)plan_row_ranges(n_cu, pp.passes, WT, LS_THREADS / 64, 2, 0);
  p.passes = (unsigned)pp.passes;
  p.lds = (size_t)K * pp.rows * 6 + 4 * (size_t)pp.rows + 16 * 48 + 16;
  p.rows_per_pass = pp.rows;
  return p;
}
inline ResidentPlan plan_f16x3_resident(long long M, int N, int K, bool presplit, int n_cu, const UnivsConfig& cfg) {
  ResidentPlan p{};
  int r_cap = (int)std::min<long long>(RESIDENT_LDS_CAP / ((long long)K * 4 + 12), 16 * L3_MAX_RB);
  r_cap -= r_cap % 16;                                     // the LDS image holds whole 16-feature blocks
  if (cfg.linear_rows_per_pass >= 16) r_cap = std::min(r_cap, cfg.linear_rows_per_pass - cfg.linear_rows_per_pass % 16);
  if (r_cap < 16) return p;
  const PassPlan pp = plan_passes(N, r_cap, 4);
  // PRE: the slab is requested all at once, L3_WPT units per thread (cannot fail for K <= 768: <= 20 units)
  if (presplit && ((K >> 3) * 2 + (L3_THREADS / pp.rows) - 1) / (L3_THREADS / pp.rows) > L3_WPT) return p;
  const long long WT = (M + L3_TILE_M - 1) / L3_TILE_M;
  p.covered = true;
  p.RB = pp.RB;
  p.ring = k_ring(K);
  p.gx = (unsigned)plan_row_ranges(n_cu, pp.passes, WT, L3_THREADS / 64, 2, cfg.linear_grid_x);
  p.passes = (unsigned)pp.passes;
  p.lds = (size_t)K * (16 * pp.RB) * 4 + 12 * (size_t)pp.rows + 256 + 16;
  p.rows_per_pass = pp.rows;
  return p;
}

// ---- two W-resident Linears on one stream of x (linear_pair_f16x3.hip): A on x, B on x + add[row % add_rows], both column-blocked
// and on the split image.  The passes of both problems share the grid's y: A's first, then B's; each problem's passes are the ones
// plan_f16x3_resident gives it alone (same cap, same rounding), the row ranges are dealt for the sum.  No lower bound on M: the
// staging of W is paid once for two Linears, and the launch replaces a pass over x that costs more than it at any size.
inline bool pair_covered(long long M, int N_a, int N_b, int K, long long add_rows, long long blk_rows, int blk_cols_a, int blk_cols_b) {
  if (M < 1 || N_a < 1 || N_b < 1 || add_rows < 1 || blk_rows < 1 || add_rows != blk_rows || M % add_rows != 0) return false;
  if (K != 256) return false;                              // the blocked epilogue's K (resident_covered)
  if (!fits_int32(M, std::max(K, std::max(N_a, N_b)))) return false;   // (add_rows <= M: the table fits with x)
  return blocked_ok(M, N_a, (int)blk_rows, blk_cols_a) && blocked_ok(M, N_b, (int)blk_rows, blk_cols_b);
}
struct PairPlan {
  bool covered;
  int RB[2], ring;               // linear_pair_f16x3<RB of A, RB of B, ring>
  unsigned gx, passes[2];        // grid: gx x (passes[0] + passes[1])
  size_t lds;                    // the larger of the two slabs
  int rows_per_pass[2];
};
inline PairPlan plan_f16x3_pair(long long M, int N_a, int N_b, int K, int n_cu) {
  PairPlan p{};
  int r_cap = (int)std::min<long long>(RESIDENT_LDS_CAP / ((long long)K * 4 + 12), 16 * L3_MAX_RB);
  r_cap -= r_cap % 16;
  if (r_cap < 16 || k_ring(K) == 0) return p;
  const int Ns[2] = {N_a, N_b};
  for (int i = 0; i < 2; ++i) {
    const PassPlan pp = plan_passes(Ns[i], r_cap, 4);
    if (((K >> 3) * 2 + (L3_THREADS / pp.rows) - 1) / (L3_THREADS / pp.rows) > L3_WPT) return p;   // the slab is requested all at once
    p.RB[i] = pp.RB;
    p.passes[i] = (unsigned)pp.passes;
    p.rows_per_pass[i] = pp.rows;
    p.lds = std::max(p.lds, (size_t)K * (16 * pp.RB) * 4 + 12 * (size_t)pp.rows + 256 + 16);
  }
  const long long WT = (M + L3_TILE_M - 1) / L3_TILE_M;
  p.ring = k_ring(K);
  // row ranges: one workgroup per CU, every wave with at least two row tiles -- and NOT rounded down to a multiple of 8 as
  // plan_row_ranges does: the kernel's XCD remap keeps a row range's passes together for any extent, and the launch is bound by the
  // work of its slowest workgroup (an A pass: 128 features), not by the memory system, so the 15 more CUs of 51 x 5 workgroups against
  // 48 x 5 on 256 CUs are worth more than the few row ranges that straddle two XCDs cost
  const long long passes = (long long)p.passes[0] + p.passes[1];
  p.gx = (unsigned)std::max<long long>(1, std::min<long long>(n_cu / passes, WT / (2 * (L3_THREADS / 64))));
  p.covered = true;
  return p;
}

// ---- the streamed kernel (gemm_f16x3_stream.hip).  XMODE 0: a Linear; 1 / 2: a convolution on an NCHW / channels-last
// operand, M = T H W pixels, N = Cout, K = taps * Cin
inline bool stream_linear_covered(long long M, int N, int K) {
  return k_ring(K) != 0 && K >= 96 && N % 4 == 0 && M >= 2048 && fits_int32(M, N) && fits_int32(M, K);
}
inline bool stream_conv_covered(long long M, int Cin, int Cout, int taps) {
  return (taps == 9 ? Cin % 128 == 0 : k_ring(Cin) != 0) && Cout % 16 == 0 && M >= 4096 && fits_int32(M, std::max(Cin, Cout));
}
// ... with the GroupNorm + ReLU of the operand folded into its load (a 1 x 1): the (scale, bias) pairs of two frames in LDS behind the
// plan's bytes; the rows of one round of a workgroup must lie in at most two frames
inline size_t gs_affine_lds(int Cin) { return (size_t)2 * Cin * 8; }
inline bool stream_affine_covered(long long HW, int Cin) { return HW >= (GS_THREADS / 64) * GS_TILE_M && Cin <= 1024; }
// ... and the instantiations that exist with it: up to four feature blocks per pass (they fit the register file with the pairs), and
// the full pass of a Cin % 128 == 0 problem, eight blocks at ring 4 (the mask-feature convolution: no more spilled than without the
// affine).  Five to seven blocks, and eight at ring 3, spill a few registers more with it: not built, the caller keeps the GroupNorm pass
constexpr bool stream_affine_plan_covered(int RB, int ring) { return RB <= 4 || (RB == 8 && ring == 4); }
struct StreamPlan {
  int RB, ring;                  // gemm_f16x3_stream<RB, ring, XMODE>
  unsigned gx, passes;
  size_t lds;
  int rows_per_pass, remap;      // GsArgs fields
};
inline StreamPlan plan_stream(int xmode, long long M, int N, int K, int n_cu, const UnivsConfig& cfg) {
  StreamPlan p{};
  // output features per pass: 128, or 64 for short tall-K problems with a narrow output (Swin stage-3 / stage-4 proj and fc2:
  // few row tiles, N <= 768 <= K -- twice the passes fill the CUs; 172 -> 126 us at 18 400 x 1536 -> 384, 60 -> 43 us at
  // 18 400 x 384 -> 384: profiles/r04_kbench_smallm_v1.txt)
  const bool narrow = xmode == 0 && N <= 768 && K >= N && M <= 32768;
  const int r_cap = cfg.linear_rows_per_pass >= 16 ? std::min(128, cfg.linear_rows_per_pass - cfg.linear_rows_per_pass % 16)
                                                   : (narrow ? 64 : 128);
  const PassPlan pp = plan_passes(N, r_cap, xmode != 0 ? 16 : 4);
  const long long WT = (M + GS_TILE_M - 1) / GS_TILE_M;
  long long gx = plan_row_ranges(n_cu, pp.passes, WT, GS_THREADS / 64, 1, cfg.linear_grid_x);
  p.RB = pp.RB;
  p.ring = k_ring(K);
  p.lds = (size_t)2 * p.ring * 8 * (16 * pp.RB) * 16 + 8 * (size_t)(16 * pp.RB);
  if (GS_THREADS < 512 && cfg.linear_grid_x <= 0 && p.lds * (512 / GS_THREADS) <= 156 * 1024)      // (experiment: several workgroups per CU)
    gx = std::min<long long>(gx * (512 / GS_THREADS), std::max<long long>(1, WT / (GS_THREADS / 64)));
  p.gx = (unsigned)gx;
  p.passes = (unsigned)pp.passes;
  p.rows_per_pass = pp.rows;
  p.remap = cfg.linear_ablate == LA_NO_XCD_REMAP ? 0 : 1;  // XCD-aware (row range, pass) order
  return p;
}

// ---- the two-dimensional tiling (gemm_f16x3_tile.hip)
struct TilePlan {
  bool covered;
  int ct, rb, nslot, occ;        // gemm_f16x3_tile<CT, RB, NSLOT, OCC>
  unsigned grid;
  size_t lds;
  int tf, nf;                    // GtArgs fields: features per feature tile, feature tiles
};
constexpr bool tile_occ2(int ct, int rb) { return (ct == 3 && rb <= 3) || (ct == 4 && rb == 2); }   // <= 128 registers, <= 80 KB of LDS
inline TilePlan plan_tile(long long M, int N, int K, int n_cu, const UnivsConfig& cfg) {
  TilePlan p{};
  if (K % 64 != 0 || K < 384 || N % 4 != 0 || N < 128 || M < 2048 || !fits_int32(M, N) || !fits_int32(M, K) || !fits_int32(K, N)) return p;
  // k-steps in flight per workgroup (register slots of the loads): 4 where K allows -- with 2 a k-step took ~5 000 clocks at
  // 18 400 x 1536 -> 384, one memory latency under load: 44 KB in flight per CU, against the ~100 KB the L2 -> CU stream needs
  int nslot = K % 128 == 0 ? 4 : K % 96 == 0 ? 3 : 2;
  if (cfg.linear_ablate >= LA_TILE_NSLOT2 && cfg.linear_ablate <= LA_TILE_NSLOT4 && K % (32 * (cfg.linear_ablate - 5)) == 0)
    nslot = cfg.linear_ablate - 5;                                // kernel benchmarks
  // tile shape: the (CT, RB) with the least estimated time.  Per k-step and workgroup: the matrix pipe (two waves per SIMD), the LDS port
  // (fragment reads of the 8 waves + the stage writes, 128 B / clock) and the L2 -> CU stream (~14 B / clock and CU measured for this
  // access pattern: tools/probes/row_stride.hip).  One workgroup per CU: vector / memory phase and matrix phase add up (measured:
  // 67 + 34 us at 18 400 x 1536 -> 384 on 160 x 192 tiles); two per CU (the small tiles): the slower pipe of the pair.  Workgroups
  // beyond the full rounds run with the CU to themselves.  (tools/gemm_tile_sweep.py measures every shape / depth.)
  int best_occ = 1;
  double best_t = 1e300;
  for (int ct = 3; ct <= 5; ++ct)
    for (int rb = 2; rb <= 4; ++rb) {
      if (cfg.linear_grid_x >= 3 && cfg.linear_grid_x <= 5 && ct != cfg.linear_grid_x) continue;              // kernel benchmarks
      if (cfg.linear_rows_per_pass >= 128 && rb != std::min(4, cfg.linear_rows_per_pass / 64)) continue;
      const int nf = (N + 64 * rb - 1) / (64 * rb);
      int tf = (N + nf - 1) / nf;
      tf = (tf + 3) & ~3;
      if ((tf + 63) / 64 != rb) continue;                        // (a smaller RB covers this split)
      const int occ = tile_occ2(ct, rb) ? 2 : 1;
      const long long wgs = ((M + 32 * ct - 1) / (32 * ct)) * nf;
      const double ks = K / 32;
      const double mfma = 2.0 * ct * rb * 3 * 16;
      const double ldsc = (8.0 * (2 * ct + 2 * rb) * 1024 + 2 * ct * 2048 + tf * 128) / 128.0;
      const double mem = (32.0 * ct * 128 + tf * 128) / 14.0;
      const double t_alone = 1.1 * ks * (std::max(ldsc, mem) + mfma) + 6000.0;    // (1.1: 101 us measured against 93 modelled)
      const double t_full = occ == 2 ? ks * 2.0 * std::max(mfma, std::max(ldsc, mem)) + 6000.0 : t_alone;
      const long long full = wgs / ((long long)n_cu * occ), rem = wgs - full * n_cu * occ;
      const double t = full * t_full + (rem == 0 ? 0.0 : rem > n_cu ? t_full : t_alone);
      if (t < best_t) { best_t = t; p.ct = ct; p.rb = rb; p.nf = nf; p.tf = tf; best_occ = (occ == 2 && wgs > n_cu) ? 2 : 1; }
    }
  if (p.ct == 0) return p;
  if (p.ct == 5 && p.rb == 4 && nslot == 4) nslot = K % 96 == 0 ? 3 : 2;                                          // (registers)
  // (two workgroups per CU only where there are more workgroups than CUs; otherwise the same tile with the deeper load pipeline:
  //  4 600 x 3072 -> 768 on 128 x 128 tiles, 216 workgroups: 95 us with 3-4 k-steps in flight, 105 with 2)
  if (best_occ == 2) nslot = 2;                                                                                    // (128 registers)
  p.covered = true;
  p.nslot = nslot;
  p.occ = best_occ;
  p.grid = (unsigned)(((M + 32 * p.ct - 1) / (32 * p.ct)) * p.nf);
  p.lds = ((size_t)2 * (2 * p.ct * 128) + (size_t)2 * (8 * 64 * p.rb)) * 16 + (size_t)2 * 32 * p.ct * 4 + (size_t)2 * 64 * p.rb * 4;
  return p;
}

}  // namespace univs
