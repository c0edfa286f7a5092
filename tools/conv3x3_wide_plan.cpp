// Which kernel conv3x3_f16x3_f32 / conv3x3_nhwc_f16x3_f32 launch for a call, decided on the host from the planning headers the launchers
// include (univs_amd/csrc/gemm_plan.h: stream_conv_covered; univs_amd/csrc/conv3x3_wide_plan.h: conv3x3_wide_covered,
// plan_conv3x3_wide), and whether the wide kernel's walk -- workgroup b runs rounds b * rounds .. of the sequence, 8 wave tiles of 32
// pixels per round -- assigns every wave tile to exactly one (workgroup, round, wave), none twice, none beyond M.
// Cases from standard input, one per line:   M Cin Cout
// One line per (case, CU count 64 / 256 / 304):
//     M Cin Cout n_cu stream=<0|1> wide=<0|1> [nwg rounds lds once=<0|1> idle=<wave-tile slots past the last tile>]
// `stream`: the launchers answer the call at all (else UNIVS_ERR_NOT_IMPLEMENTED); `wide`: conv3x3_wide runs, else gemm_f16x3_stream.
// No GPU and no HIP runtime:   hipcc -O2 -std=c++17 -I include tools/conv3x3_wide_plan.cpp -o conv3x3_wide_plan
// tests/test_conv3x3_wide_cpu.py runs it.
#include <stdio.h>

#include <vector>

#include "../univs_amd/csrc/conv3x3_wide_plan.h"
using namespace univs;

// the kernel's own arithmetic (conv3x3_wide.hip: rd0, rounds, tt)
static bool covers_once(long long M, const WidePlan& p, long long* idle) {
  const int NWV = CW_THREADS / 64;
  const long long WT = (M + CW_TILE_M - 1) / CW_TILE_M, total = (WT + NWV - 1) / NWV;
  std::vector<int> tiles((size_t)WT, 0);
  *idle = 0;
  bool ok = true;
  for (unsigned wg = 0; wg < p.nwg; ++wg) {
    const long long rd0 = (long long)wg * p.rounds;
    const long long rounds = std::min<long long>(p.rounds, total - rd0);
    if (rounds <= 0) ok = false;                                 // a workgroup with nothing to do: the plan asked for too many
    for (long long rd = 0; rd < rounds; ++rd)
      for (int wave = 0; wave < NWV; ++wave) {
        const long long tt = (rd0 + rd) * NWV + wave;
        if (tt < WT) ++tiles[(size_t)tt];                        // a tile past the last one stores nothing
        else ++*idle;
      }
  }
  for (int c : tiles)
    if (c != 1) ok = false;
  return ok;
}

int main() {
  const int cus[] = {64, 256, 304};
  long long M;
  int Cin, Cout, bad = 0;
  while (scanf("%lld %d %d", &M, &Cin, &Cout) == 3)
    for (int n_cu : cus) {
      const bool stream = stream_conv_covered(M, Cin, Cout, 9), wide = conv3x3_wide_covered(M, Cin, Cout);
      printf("%lld %d %d %d stream=%d wide=%d", M, Cin, Cout, n_cu, (int)stream, (int)wide);
      if (wide) {
        const WidePlan p = plan_conv3x3_wide(M, n_cu);
        long long idle = 0;
        const bool once = covers_once(M, p, &idle);
        bad += !once || !stream || p.nwg > (unsigned)n_cu;
        printf(" %u %d %zu once=%d idle=%lld", p.nwg, p.rounds, conv3x3_wide_lds(), (int)once, idle);
      }
      printf("\n");
    }
  return bad ? 1 : 0;
}
