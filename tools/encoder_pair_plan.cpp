// What linear_pair_f16x3 (univs_amd/csrc/linear_pair_f16x3.hip) launches, decided on the host from the planning header its launcher
// includes (univs_amd/csrc/gemm_plan.h: pair_covered, plan_f16x3_pair), and whether that grid covers the two problems: the kernel's own
// index arithmetic -- XCD remap of the linear workgroup id, (row range, pass), problem and first feature of the pass, row tiles of the
// row range, tiles of each wave -- is restated here and every (32-row tile, 4-feature group) of both outputs is counted.
// Cases from standard input, one per line:   M N_a N_b K
// One line per (case, CU count 64 / 256 / 304):
//     M N_a N_b K n_cu linear_pair_f16x3<RBa,RBb,ring> gx passes_a passes_b lds once=<0|1>       or     ... not covered
// `once` = 1: every cell of both outputs is written by exactly one (workgroup, wave).
// No GPU and no HIP runtime:   hipcc -O2 -std=c++17 -I include tools/encoder_pair_plan.cpp -o encoder_pair_plan
// tests/test_encoder_pair_cpu.py runs it.
#include <stdio.h>

#include <vector>

#include "../univs_amd/csrc/gemm_plan.h"
using namespace univs;

static unsigned xcd_remap(unsigned bid, unsigned nblocks) {   // common.h
  const unsigned nx = 8;
  const unsigned q = nblocks / nx, r = nblocks % nx;
  const unsigned xcd = bid % nx, idx = bid / nx;
  const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

static bool covers_once(long long M, const int (&N)[2], const PairPlan& p) {
  const int WT = (int)((M + L3_TILE_M - 1) / L3_TILE_M), NWV = L3_THREADS / 64;
  const unsigned gy = p.passes[0] + p.passes[1];
  std::vector<int> cells[2];
  for (int i = 0; i < 2; ++i) cells[i].assign((size_t)WT * (N[i] / 4), 0);
  for (unsigned by_ = 0; by_ < gy; ++by_)
    for (unsigned bx_ = 0; bx_ < p.gx; ++bx_) {
      const unsigned lw = xcd_remap(bx_ + p.gx * by_, p.gx * gy);
      const unsigned bx = lw / gy, by = lw - bx * gy;
      const int prob = by < p.passes[0] ? 0 : 1;
      const int n0 = (int)(prob ? by - p.passes[0] : by) * p.rows_per_pass[prob];
      const int R = std::min(p.rows_per_pass[prob], N[prob] - n0);
      if (R < 4 || R % 4 != 0 || R > 16 * p.RB[prob]) return false;
      const int wg0 = (int)((long long)WT * bx / p.gx), wg1 = (int)((long long)WT * (bx + 1) / p.gx);
      for (int wave = 0; wave < NWV; ++wave) {
        const int wt0 = wg0 + wave;
        const int ntiles = wt0 < wg1 ? (wg1 - wt0 + NWV - 1) / NWV : 0;
        for (int t = 0; t < ntiles; ++t)
          for (int f = 0; f < R; f += 4) ++cells[prob][(size_t)(wt0 + t * NWV) * (N[prob] / 4) + (n0 + f) / 4];
      }
    }
  for (int i = 0; i < 2; ++i)
    for (int c : cells[i])
      if (c != 1) return false;
  return true;
}

int main() {
  const int cus[] = {64, 256, 304};
  long long M;
  int N[2], K, bad = 0;
  while (scanf("%lld %d %d %d", &M, &N[0], &N[1], &K) == 4)
    for (int n_cu : cus) {
      printf("%lld %d %d %d %d ", M, N[0], N[1], K, n_cu);
      const PairPlan p = plan_f16x3_pair(M, N[0], N[1], K, n_cu);
      if (!pair_covered(M, N[0], N[1], K, M, M, 4, 4) || !p.covered) {
        printf("not covered\n");
        continue;
      }
      const bool once = covers_once(M, N, p);
      bad += !once;
      printf("linear_pair_f16x3<%d,%d,%d> %u %u %u %zu once=%d\n", p.RB[0], p.RB[1], p.ring, p.gx, p.passes[0], p.passes[1], p.lds, (int)once);
    }
  return bad ? 1 : 0;
}
