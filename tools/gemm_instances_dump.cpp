// Which kernel instantiation each case of tests/gemm_instances.py runs, decided on the host from the planning header the launchers
// include (univs_amd/csrc/gemm_plan.h) and printed at 64, 256 and 304 CUs, one line per (case, CU count):  <id> <n_cu> <instantiation>
// The cases are read from standard input, one per line (tests/gemm_instances.py: plan_line), the settings being UnivsConfig's
// linear_rows_per_pass / linear_grid_x / linear_ablate:
//     resident <id> M N K epi blk_rows blk_cols pre terms rows_per_pass grid_x ablate     univs_linear_fused_f32 / _blocked_f32 (pre: *_presplit)
//     presplit <id> M N K epi rows_per_pass grid_x ablate                                 univs_linear_presplit_f32: the tiled kernel, else the streamed
//     conv     <id> xmode taps T Cin Cout H W affine rows_per_pass grid_x ablate          the convolutions on the streamed kernel
//     mlp      <id> M C Hd act ablate                                                     univs_mlp_presplit_v2_f32
// No GPU and no HIP runtime:   hipcc -O2 -std=c++17 -I include tools/gemm_instances_dump.cpp -o gemm_instances_dump
// tests/test_gemm_instances_cpu.py asserts that every case yields the instantiation it names at all three CU counts.
#include <stdio.h>
#include <string.h>

#include "../univs_amd/csrc/gemm_plan.h"
using namespace univs;

static UnivsConfig config_of(int terms, int rows_per_pass, int grid_x, int ablate) {
  UnivsConfig c{};
  c.size = (int)sizeof(UnivsConfig);
  c.linear_terms = terms;
  c.linear_rows_per_pass = rows_per_pass;
  c.linear_grid_x = grid_x;
  c.linear_ablate = ablate;
  return c;
}

// linear_split_f32 (linear_split.hip) -> linear_f16x3_f32 (linear_f16x3.hip)
static void resident(char* out, size_t n, long long M, int N, int K, int epi, int blk_rows, int blk_cols, int pre, const UnivsConfig& cfg, int n_cu) {
  snprintf(out, n, "not covered");
  if (!resident_covered(M, N, K, epi, blk_rows, blk_cols)) return;
  const bool six = resident_six_products(cfg, pre != 0);
  const ResidentPlan p = six ? plan_bf16x6_resident(M, N, K, epi, n_cu) : plan_f16x3_resident(M, N, K, pre != 0, n_cu, cfg);
  if (!p.covered) return;
  if (six) snprintf(out, n, "linear_bf16x6<%d,%d,%d,%d>", p.RB, epi == EPI_BLOCKED ? 8 : p.ksc, epi == EPI_BLOCKED ? 4 : p.ring, epi);
  else snprintf(out, n, "linear_f16x3<%d,%d,%d>", p.RB, p.ring, pre ? 1 : 0);
}

// univs_linear_presplit_f32 (capi.hip): linear_f16x3_tile_f32 unless linear_ablate == LA_NO_TILE or not covered, then linear_f16x3_stream_f32
static void presplit(char* out, size_t n, long long M, int N, int K, const UnivsConfig& cfg, int n_cu) {
  snprintf(out, n, "not covered");
  if (cfg.linear_ablate != univs::LA_NO_TILE) {
    const TilePlan t = plan_tile(M, N, K, n_cu, cfg);
    if (t.covered) {
      // the launcher's switch: two workgroups per CU only for the tiles built with them, then two load slots
      const bool occ2 = tile_occ2(t.ct, t.rb) && t.occ == 2;
      snprintf(out, n, "gemm_f16x3_tile<%d,%d,%d,%d>", t.ct, t.rb, occ2 ? 2 : (t.nslot == 4 || t.nslot == 3 ? t.nslot : 2), occ2 ? 2 : 1);
      return;
    }
  }
  if (!stream_linear_covered(M, N, K)) return;
  const StreamPlan p = plan_stream(0, M, N, K, n_cu, cfg);
  snprintf(out, n, "gemm_f16x3_stream<%d,%d,0>", p.RB, p.ring);
}

// gs_conv (gemm_f16x3_stream.hip)
static void conv(char* out, size_t n, int xmode, int taps, int T, int Cin, int Cout, int H, int W, int affine, const UnivsConfig& cfg, int n_cu) {
  snprintf(out, n, "not covered");
  const long long M = (long long)T * H * W;
  if (!stream_conv_covered(M, Cin, Cout, taps)) return;
  if (affine && (taps != 1 || !stream_affine_covered((long long)H * W, Cin))) return;
  const StreamPlan p = plan_stream(xmode, M, Cout, taps * Cin, n_cu, cfg);
  if (affine && !stream_affine_plan_covered(p.RB, p.ring)) return;
  if (affine) snprintf(out, n, "gemm_f16x3_stream<%d,%d,%d,1>", p.RB, p.ring, xmode);
  else snprintf(out, n, "gemm_f16x3_stream<%d,%d,%d>", p.RB, p.ring, xmode);
}

// mlp_f16x3_f32 / ml_launch (mlp_f16x3.hip): the width picks <KS1, CT, NW, DB>, the activation ACT; linear_ablate 2 / 3 / 4 the timing
// ablations of the encoder FFN (C = 256, ReLU) and Swin stage 1 (C = 96, GELU), 10 the phase-shifted kernel where it is built
static void mlp(char* out, size_t n, long long M, int C, int Hd, int act, int ablate) {
  snprintf(out, n, "not covered");
  if ((act != 1 && act != 2) || Hd < 32 || Hd % 32 != 0 || M < 2048 || M * (long long)C * 4 >= 0x7FFFFFFFLL) return;
  int ct, nw, db;
  switch (C) {
    case 96: ct = 2; nw = 4; db = 1; break;
    case 128: case 192: case 256: ct = 1; nw = 8; db = 1; break;
    case 384: ct = 1; nw = 4; db = 0; break;
    default: return;
  }
  const int ks1 = C / 32;
  if ((size_t)(db ? 2 : 1) * 16 * C * 16 + (size_t)(2 * Hd + 6 * C) * 4 > 160 * 1024) return;
  int abl = 0;
  if (ablate >= univs::LA_MLP_NOMFMA && ablate <= univs::LA_MLP_NOACT && ((ks1 == 8 && act == 1) || (ks1 == 3 && act == 2))) abl = ablate - 1;
  if (abl == 0 && ablate == univs::LA_MLP_PHASE_SHIFT && db && nw == 8 && ct == 1 && ks1 >= 4 && (size_t)4 * 8 * C * 16 + (size_t)(2 * Hd + 6 * C) * 4 <= 160 * 1024) {
    snprintf(out, n, "mlp_f16x3_ps<%d,%d>", ks1, act);
    return;
  }
  snprintf(out, n, "mlp_f16x3<%d,%d,%d,%d,%d,%d>", ks1, ct, act, nw, abl, db);
}

int main() {
  const int cus[] = {64, 256, 304};
  char line[512], kind[32], id[128], inst[96];
  int bad = 0;
  while (fgets(line, sizeof(line), stdin)) {
    if (line[0] == '#' || line[0] == '\n') continue;
    long long M;
    int N, K, epi, br, bc, pre, terms, rpp, gx, abl, xmode, taps, T, Cin, Cout, H, W, aff, C, Hd, act;
    if (sscanf(line, "%31s %127s", kind, id) != 2) { ++bad; continue; }
    const char* rest = strstr(line, id) + strlen(id);
    for (int n_cu : cus) {
      if (!strcmp(kind, "resident") && sscanf(rest, "%lld %d %d %d %d %d %d %d %d %d %d", &M, &N, &K, &epi, &br, &bc, &pre, &terms, &rpp, &gx, &abl) == 11)
        resident(inst, sizeof(inst), M, N, K, epi, br, bc, pre, config_of(terms, rpp, gx, abl), n_cu);
      else if (!strcmp(kind, "presplit") && sscanf(rest, "%lld %d %d %d %d %d %d", &M, &N, &K, &epi, &rpp, &gx, &abl) == 7)
        presplit(inst, sizeof(inst), M, N, K, config_of(0, rpp, gx, abl), n_cu);
      else if (!strcmp(kind, "conv") && sscanf(rest, "%d %d %d %d %d %d %d %d %d %d %d", &xmode, &taps, &T, &Cin, &Cout, &H, &W, &aff, &rpp, &gx, &abl) == 11)
        conv(inst, sizeof(inst), xmode, taps, T, Cin, Cout, H, W, aff, config_of(0, rpp, gx, abl), n_cu);
      else if (!strcmp(kind, "mlp") && sscanf(rest, "%lld %d %d %d %d", &M, &C, &Hd, &act, &abl) == 5)
        mlp(inst, sizeof(inst), M, C, Hd, act, abl);
      else { ++bad; snprintf(inst, sizeof(inst), "unreadable case line"); }
      printf("%s %d %s\n", id, n_cu, inst);
    }
  }
  return bad ? 1 : 0;
}
