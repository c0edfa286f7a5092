// Which kernel the entry univs_encoder_linear_pair_presplit_f32 launches for a call, decided on the host from the planning headers the
// launchers include (univs_amd/csrc/gemm_plan.h: pair_covered, plan_f16x3_pair; univs_amd/csrc/pair_xres_plan.h: pair_xres_covered), and
// whether the x-resident kernel's walk -- workgroups persistent over the groups of 128 rows, 16 rows per wave, chunks of 32 features --
// writes every (row, 4-feature group) of both outputs exactly once.
// Cases from standard input, one per line:   M N_a N_b K add_rows blk_rows blk_cols_a blk_cols_b
// One line per (case, CU count 64 / 256 / 304):
//     M N_a N_b K n_cu entry=<0|1> xres=<0|1> [grid lds once=<0|1>]
// `entry`: the entry answers the call at all (else UNIVS_ERR_NOT_IMPLEMENTED); `xres`: linear_pair_xres runs, else linear_pair_f16x3.
// No GPU and no HIP runtime:   hipcc -O2 -std=c++17 -I include tools/encoder_xres_plan.cpp -o encoder_xres_plan
// tests/test_encoder_pair_xres_cpu.py runs it.
#include <stdio.h>

#include <vector>

#include "../univs_amd/csrc/pair_xres_plan.h"
using namespace univs;

static bool covers_once(long long M, const int (&N)[2], unsigned nwg) {
  const int ngroups = (int)((M + PX_ROWS - 1) / PX_ROWS), NWV = PX_THREADS / 64;
  std::vector<int> cells[2];
  for (int i = 0; i < 2; ++i) cells[i].assign((size_t)M * (N[i] / 4), 0);
  for (unsigned wg = 0; wg < nwg; ++wg)
    for (int grp = (int)wg; grp < ngroups; grp += (int)nwg)
      for (int wave = 0; wave < NWV; ++wave)
        for (int j = 0; j < 16; ++j) {
          const long long m = (long long)grp * PX_ROWS + wave * 16 + j;
          if (m >= M) continue;                               // rows past the end store nothing
          for (int i = 0; i < 2; ++i)
            for (int c = 0; c < N[i] / PX_CHUNK; ++c)
              for (int f = 0; f < PX_CHUNK; f += 4) ++cells[i][(size_t)m * (N[i] / 4) + (PX_CHUNK * c + f) / 4];
        }
  for (int i = 0; i < 2; ++i)
    for (int c : cells[i])
      if (c != 1) return false;
  return true;
}

int main() {
  const int cus[] = {64, 256, 304};
  long long M, add_rows, blk_rows;
  int N[2], K, ca, cb, bad = 0;
  while (scanf("%lld %d %d %d %lld %lld %d %d", &M, &N[0], &N[1], &K, &add_rows, &blk_rows, &ca, &cb) == 8)
    for (int n_cu : cus) {
      const PairPlan p = plan_f16x3_pair(M, N[0], N[1], K, n_cu);
      const bool entry = pair_covered(M, N[0], N[1], K, add_rows, blk_rows, ca, cb) && p.covered && p.RB[0] == 8 && p.RB[1] == 6 && p.ring == 4;
      const bool xres = pair_xres_covered(M, N[0], N[1], K, add_rows, blk_rows, ca, cb, n_cu);
      printf("%lld %d %d %d %d entry=%d xres=%d", M, N[0], N[1], K, n_cu, (int)entry, (int)xres);
      if (xres) {
        const unsigned nwg = pair_xres_grid(M, n_cu);
        const bool once = covers_once(M, N, nwg);
        bad += !once || !entry;
        printf(" %u %zu once=%d", nwg, pair_xres_lds(N[0], N[1], K), (int)once);
      }
      printf("\n");
    }
  return bad ? 1 : 0;
}
