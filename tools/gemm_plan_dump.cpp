// What the launchers of the three-product GEMM family decide, printed one line per (case, kernel) on the host: which kernel
// instantiation, grid, workgroup size, dynamic LDS bytes and the kernel-argument fields computed on the host -- from the
// planning header the launchers include (univs_amd/csrc/gemm_plan.h).  No GPU and no HIP runtime:
//     hipcc -O2 -std=c++17 -I include tools/gemm_plan_dump.cpp -o gemm_plan_dump && ./gemm_plan_dump
// tests/test_gemm_plan_cpu.py compares the output with tests/gemm_plan_table.txt.
// -DGEMM_PLAN_DUMP_PLANNERS='"file"' replaces the four dump_* functions below by those of `file`: the way to run ANOTHER
// statement of the launch logic (a transcription of earlier launchers, a proposed change) over the same cases.
#include <stdio.h>
#include <string.h>

#include "../include/univs_hip.h"

struct Ctx {
  int n_cu;
  UnivsConfig cfg;
};
static void section(const char* label) {   // the label once, as a header line in front of its cases
  static char last[96] = "";
  if (strcmp(last, label) != 0) printf("# %s\n", label);
  snprintf(last, sizeof(last), "%s", label);
}
static void emit_uncovered(const char* label, const char* kernel, const char* shape) {
  section(label);
  printf("%s | %s -> not covered\n", shape, kernel);
}
static void emit_launch(const char* label, const char* shape, const char* inst, unsigned gx, unsigned gy, int block, size_t lds,
                        const char* fields) {
  section(label);
  printf("%s -> %s grid=(%u,%u) block=%d lds=%zu %s\n", shape, inst, gx, gy, block, lds, fields);
}
static const char* shape_mnk(char (&buf)[160], long long M, int N, int K, int epi) {
  snprintf(buf, sizeof(buf), "M=%lld N=%d K=%d epi=%d", M, N, K, epi);
  return buf;
}

#ifdef GEMM_PLAN_DUMP_PLANNERS
#include GEMM_PLAN_DUMP_PLANNERS
#else
#include "../univs_amd/csrc/gemm_plan.h"
using namespace univs;

// univs_linear_fused_f32 / _blocked_f32 (presplit: their *_presplit siblings); UnivsConfig.linear_terms picks the arithmetic
static void dump_resident(const char* label, const Ctx& c, long long M, int N, int K, int epi, int blk_rows, int blk_cols, bool presplit) {
  char sh[160], inst[96], fields[96];
  snprintf(sh, sizeof(sh), "M=%lld N=%d K=%d epi=%d blk=%dx%d pre=%d terms=%d", M, N, K, epi, blk_rows, blk_cols, (int)presplit, c.cfg.linear_terms);
  const bool six = resident_six_products(c.cfg, presplit);
  if (!resident_covered(M, N, K, epi, blk_rows, blk_cols)) return emit_uncovered(label, "resident", sh);
  const ResidentPlan p = six ? plan_bf16x6_resident(M, N, K, epi, c.n_cu) : plan_f16x3_resident(M, N, K, presplit, c.n_cu, c.cfg);
  if (!p.covered) return emit_uncovered(label, "resident", sh);
  if (six) snprintf(inst, sizeof(inst), "linear_bf16x6<%d,%d,%d,%d>", p.RB, p.ksc, p.ring, epi);
  else snprintf(inst, sizeof(inst), "linear_f16x3<%d,%d,%d>", p.RB, p.ring, (int)presplit);
  if (six) snprintf(fields, sizeof(fields), "rows_per_pass=%d", p.rows_per_pass);
  else snprintf(fields, sizeof(fields), "rows_per_pass=%d ablate=%d", p.rows_per_pass, c.cfg.linear_ablate);
  emit_launch(label, sh, inst, p.gx, p.passes, six ? LS_THREADS : L3_THREADS, p.lds, fields);
}
static void dump_stream_plan(const char* label, const Ctx& c, const char* sh, int xmode, long long M, int N, int K) {
  char inst[96], fields[96];
  const StreamPlan p = plan_stream(xmode, M, N, K, c.n_cu, c.cfg);
  snprintf(inst, sizeof(inst), "gemm_f16x3_stream<%d,%d,%d>", p.RB, p.ring, xmode);
  snprintf(fields, sizeof(fields), "rows_per_pass=%d remap=%d", p.rows_per_pass, p.remap);
  emit_launch(label, sh, inst, p.gx, p.passes, GS_THREADS, p.lds, fields);
}
// univs_linear_presplit_f32 with the tiled kernel switched off (or not covering)
static void dump_stream(const char* label, const Ctx& c, long long M, int N, int K) {
  char sh[160];
  shape_mnk(sh, M, N, K, 0);
  if (!stream_linear_covered(M, N, K)) return emit_uncovered(label, "stream", sh);
  dump_stream_plan(label, c, sh, 0, M, N, K);
}
// kind 0 / 1: univs_conv3x3_presplit_f32 / _nhwc_; 2: univs_conv1x1_presplit_f32
static void dump_conv(const char* label, const Ctx& c, int kind, int T, int Cin, int Cout, int H, int W) {
  char sh[160];
  snprintf(sh, sizeof(sh), "conv kind=%d T=%d Cin=%d Cout=%d H=%d W=%d", kind, T, Cin, Cout, H, W);
  const long long M = (long long)T * H * W;
  const int taps = kind == 2 ? 1 : 9;
  if (!stream_conv_covered(M, Cin, Cout, taps)) return emit_uncovered(label, "stream", sh);
  dump_stream_plan(label, c, sh, kind == 1 ? 2 : 1, M, Cout, taps * Cin);
}
// univs_linear_presplit_f32: the tiled kernel
static void dump_tile(const char* label, const Ctx& c, long long M, int N, int K) {
  char sh[160], inst[96], fields[96];
  shape_mnk(sh, M, N, K, 0);
  const TilePlan p = plan_tile(M, N, K, c.n_cu, c.cfg);
  if (!p.covered) return emit_uncovered(label, "tile", sh);
  snprintf(inst, sizeof(inst), "gemm_f16x3_tile<%d,%d,%d,%d>", p.ct, p.rb, p.nslot, p.occ);
  snprintf(fields, sizeof(fields), "tf=%d nf=%d", p.tf, p.nf);
  emit_launch(label, sh, inst, p.grid, 1u, GT_THREADS, p.lds, fields);
}
#endif

// ---- cases
static Ctx ctx(int n_cu, int rows_per_pass = 0, int grid_x = 0, int ablate = 0) {
  Ctx c{};
  c.n_cu = n_cu;
  c.cfg.size = (int)sizeof(UnivsConfig);
  c.cfg.linear_rows_per_pass = rows_per_pass;
  c.cfg.linear_grid_x = grid_x;
  c.cfg.linear_ablate = ablate;
  return c;
}
// which kernels a Linear case is put through: the resident kernel on pre-split W / on raw W / with six products, the streamed, the tiled
enum { R = 1, W = 2, S = 4, T = 8, L = 16, ALL = 31 };
// the kernels whose K range holds K (resident: K <= 768; tiled: K >= 384; streamed: where ops.py routes it, K >= 384); the
// ranges' own edges are cases with an explicit mask
static int by_k(int K) { return (K <= 768 ? R | S : 0) | (K >= 384 ? T | L : 0); }
static void linear(const char* label, Ctx c, int mask, long long M, int K, int N, int epi = 0, int blk_cols = 0, int blk_rows = 0) {
  if (mask & R) dump_resident(label, c, M, N, K, epi, blk_rows, blk_cols, true);
  if (mask & W) dump_resident(label, c, M, N, K, epi, blk_rows, blk_cols, false);
  c.cfg.linear_terms = 6;
  if (mask & S) dump_resident(label, c, M, N, K, epi, blk_rows, blk_cols, false);
  c.cfg.linear_terms = 0;
  if (epi == 4) return;
  if (mask & T) dump_stream(label, c, M, N, K);
  if (mask & L) dump_tile(label, c, M, N, K);
}
struct Lin {
  int M, K, N, epi;
};

// the launches of tools/gemmset.py (`more`: kernels beyond those of by_k)
static void gemmset(const char* label, const Ctx& c, int T_, int more) {
  const int S_ = 19320;
  linear(label, c, R | S | more, (long long)T_ * S_, 256, 256, 4, 16, S_);
  linear(label, c, R | S | more, (long long)T_ * S_, 256, 288, 4, 36, S_);
  const Lin s[] = {{S_, 256, 256, 3}, {184 * 320, 96, 288, 0}, {184 * 320, 96, 96, 3}, {92 * 160, 192, 576, 0}, {92 * 160, 192, 192, 3},
                   {3680, 384, 1152, 0}, {3680, 384, 384, 3}, {3680, 384, 1536, 2}, {3680, 1536, 384, 3}, {920, 768, 2304, 0}, {920, 768, 768, 3},
                   {920, 768, 3072, 2}, {920, 3072, 768, 3}, {92 * 160, 384, 192, 0}, {3680, 768, 384, 0}, {920, 1536, 768, 0}, {14720, 256, 768, 0},
                   {3680, 256, 768, 0}, {920, 256, 768, 0}};
  for (auto& t : s) linear(label, c, by_k(t.K) | (t.K <= 768 ? more : 0), (long long)T_ * t.M, t.K, t.N, t.epi);
  dump_conv(label, c, 0, T_, 256, 256, 184, 320);
  dump_conv(label, c, 1, T_, 256, 256, 184, 320);
  dump_conv(label, c, 2, T_, 256, 256, 184, 320);
  dump_conv(label, c, 2, T_, 96, 256, 184, 320);
}
// the Linears of a Swin backbone (univs_amd/workloads.py: embedding width E, T frames padded to Hp x Wp), three products
static void swin(const char* label, const Ctx& c, int E, int T_, int Hp, int Wp) {
  for (int s = 0; s < 4; ++s) {
    const int C = E << s;
    const long long M = (long long)T_ * ((Hp / 4) >> s) * ((Wp / 4) >> s);
    linear(label, c, by_k(C) & ~S, M, C, 3 * C);
    linear(label, c, by_k(C) & ~S, M, C, C, 3);
    linear(label, c, by_k(C) & ~S, M, C, 4 * C, 2);
    linear(label, c, by_k(4 * C) & ~S, M, 4 * C, C, 3);
    if (s < 3) linear(label, c, by_k(4 * C) & ~S, M / 4, 4 * C, 2 * C);
  }
}

int main() {
  const Ctx c = ctx(256);
  gemmset("gemmset T=5", c, 5, W);
  swin("cfg4 Swin-B", c, 128, 5, 736, 1280);
  swin("cfg5 Swin-L", c, 192, 10, 1088, 1920);

  // ---- the shapes of the family's GPU tests (tests/test_ops_gpu.py), those the sections above hold already left out
  {
    const char* l = "test_linear_blocked";
    const int nsc[4][3] = {{5, 19320, 32}, {5, 19320, 36}, {2, 4200, 48}, {3, 2352, 16}};
    for (auto& t : nsc) linear(l, c, R | S, (long long)t[0] * t[1], 256, t[2] == 16 || t[2] == 32 ? 256 : 8 * t[2], 4, t[2], t[1]);
    for (int N : {256, 288}) linear(l, c, R | S, 96600, 256, N);   // the standard-layout Linear it is compared with
    linear(l, c, R | S, 8400, 256, 384);
    linear(l, c, R | S, 7056, 256, 256);
  }
  {
    const char* l = "test_linear_split / _fused / _resident_presplit / _row_scaling";
    const Lin s[] = {{5000, 256, 1024, 1}, {4099, 128, 100, 0}, {2048, 384, 4, 0}, {3000, 256, 108, 1}, {4096, 256, 288, 0}, {58880, 96, 288, 0},
                     {58880, 96, 384, 2}, {14720, 384, 96, 3}, {14720, 192, 576, 0}, {14720, 192, 768, 2}, {3680, 768, 192, 3}, {3680, 384, 1536, 2},
                     {4099, 96, 100, 1}, {2500, 768, 2304, 0}, {19320, 1024, 256, 0}, {4600, 1536, 384, 3}, {4613, 3072, 768, 2}, {5000, 1024, 128, 1},
                     {73600, 256, 768, 0}, {2048, 96, 128, 0}, {2049, 128, 520, 2}, {2048, 768, 132, 1}, {2048, 768, 124, 3}};
    for (auto& t : s) linear(l, c, by_k(t.K), t.M, t.K, t.N, t.epi);
    // test_linear_resident_presplit: the same launches on raw W (the gemmset section holds its other shapes on raw W)
    const Lin w[] = {{58880, 96, 288, 0}, {14720, 192, 576, 0}, {4099, 96, 100, 1}, {2048, 384, 4, 0}, {73600, 256, 768, 0}};
    for (auto& t : w) linear(l, c, W, t.M, t.K, t.N, t.epi);
    linear(l, c, R | W, 5003, 1024, 208, 3);   // test_presplit_weights: K > 768 without the streamed route
    // test_linear_split_uncovered_shapes_return_none
    linear(l, c, R | S | T, 4096, 80, 96);
    linear(l, c, ALL & ~W, 4096, 1024, 6);
    linear(l, c, R | S | T, 4096, 256, 6);
    linear(l, c, R | S | T, 100, 256, 8);
  }
  {
    const char* l = "test_linear_tile_kernel / test_streamed_linear / test_presplit_weights";
    const Lin s[] = {{18400, 384, 384, 3}, {18400, 768, 384, 0}, {18399, 768, 200, 1}, {2049, 384, 132, 3}, {4100, 576, 260, 0}, {4100, 1152, 256, 3},
                     {73600, 384, 192, 0}, {4100, 960, 72, 0}, {3000, 864, 136, 1}, {2500, 2304, 264, 2}, {70000, 768, 192, 0}, {5003, 1024, 208, 3},
                     {4096, 1024, 256, 0}};
    for (auto& t : s) linear(l, c, T | L, t.M, t.K, t.N, t.epi);
  }
  {
    const char* l = "test_mlp_fused: the two Linears it is compared with";
    const int s[][5] = {{19320, 256, 1024, 1, 0}, {58880, 96, 384, 2, 3}, {14720, 192, 768, 2, 3}, {5000, 128, 512, 2, 3}, {4099, 96, 384, 2, 0},
                        {2049, 256, 32, 1, 3}, {3000, 256, 2048, 2, 0}, {2048, 192, 96, 1, 0}, {18400, 384, 1536, 2, 3}, {2100, 384, 64, 1, 0}};
    for (auto& t : s) {
      linear(l, c, by_k(t[1]) & ~S, t[0], t[1], t[2], t[3]);
      linear(l, c, by_k(t[2]) & ~S, t[0], t[2], t[1], t[4]);
    }
  }
  {
    const char* l = "test_conv3x3 / test_conv1x1";
    const int s3[][5] = {{2, 256, 256, 48, 44}, {1, 128, 128, 70, 64}, {3, 256, 256, 17, 83}, {1, 384, 256, 64, 64}, {1, 128, 16, 64, 64},
                         {1, 96, 64, 64, 64}, {1, 128, 128, 16, 16}};
    for (auto& t : s3) dump_conv(l, c, 0, t[0], t[1], t[2], t[3], t[4]);
    dump_conv(l, c, 1, 2, 128, 64, 46, 80);
    dump_conv(l, c, 0, 2, 128, 64, 46, 80);
    dump_conv(l, c, 1, 2, 96, 64, 46, 80);
    const int s1[][5] = {{2, 256, 256, 92, 160}, {3, 96, 256, 60, 77}, {1, 192, 256, 46, 93}, {2, 384, 256, 46, 80}, {5, 768, 256, 23, 40}, {1, 128, 64, 70, 70},
                         {1, 128, 16, 64, 64}, {1, 80, 64, 64, 64}, {1, 128, 128, 16, 16}};
    for (auto& t : s1) dump_conv(l, c, 2, t[0], t[1], t[2], t[3], t[4]);
  }

  // ---- the edges
  for (int K : {96, 128, 192, 256, 384, 512, 768, 864, 960, 1536, 2304, 3072}) linear("edge K", c, by_k(K), 18400, K, 384);
  for (int K : {64, 160, 320, 448, 800}) linear("edge K: no ring, or the tiled kernel alone", c, ALL & ~W, 18400, K, 256);
  linear("edge K: the ranges of the resident and the tiled kernel", c, R | S, 18400, 896, 256);
  linear("edge K: the ranges of the resident and the tiled kernel", c, L, 18400, 256, 256);
  // every RB from 1 to 8 (7 with six products), short last passes, a last pass that is no multiple of 16, N % 4
  for (int N : {4, 16, 20, 32, 48, 64, 80, 96, 100, 104, 108, 112, 128, 132, 260, 1028, 1030}) linear("edge N", c, R | S, 40000, 256, N);
  for (int N : {4, 16, 32, 36, 48, 68, 84, 100, 124, 128, 132, 1028}) linear("edge N", c, T | L, 40000, 768, N);
  for (int N : {16, 64, 80, 128, 144, 272}) dump_conv("edge N", c, 0, 1, 128, N, 80, 80);
  // pass counts on both sides of "rounding down to a multiple of 8 idles more than a tenth of the CUs"
  for (int p = 1; p <= 20; ++p) linear("edge passes of 128 features", c, R, 96600, 256, 128 * p);
  for (int p : {2, 3, 6, 7, 13, 16, 17, 19}) linear("edge passes of 104 features, six products", c, S, 96600, 256, 104 * p);
  for (int p : {1, 2, 3, 6, 7, 12}) linear("edge passes of 64 features (narrow)", c, T, 30000, 128 * ((64 * p + 127) / 128), 64 * p);
  // the fewest rows the kernels take
  for (int M : {2016, 2017}) linear("edge M", c, R | S, M, 256, 256);
  for (int M : {2047, 2048, 2049}) linear("edge M", c, T | L, M, 768, 192);
  for (int Wd : {4095, 4096, 4097}) {
    dump_conv("edge M", c, 2, 1, 128, 64, 1, Wd);
    dump_conv("edge M", c, 0, 1, 128, 64, 1, Wd);
  }
  // the extent limits of 32-bit offsets
  linear("edge 2^31", c, R | S, 2097151, 256, 256);
  linear("edge 2^31", c, R | S, 2097152, 256, 256);
  linear("edge 2^31", c, T | L, 699050, 768, 128);
  linear("edge 2^31", c, T | L, 699051, 768, 128);
  linear("edge 2^31", c, T | L, 4096, 24576, 21840);
  linear("edge 2^31", c, T | L, 4096, 24576, 21848);
  dump_conv("edge 2^31", c, 2, 1, 256, 64, 2048, 1023);
  dump_conv("edge 2^31", c, 2, 1, 256, 64, 2048, 1024);
  // 64 features per pass for short tall-K problems with a narrow output
  for (int M : {32768, 32769}) {
    linear("edge narrow", c, T, M, 768, 768);
    linear("edge narrow", c, T, M, 768, 772);
    linear("edge narrow", c, T, M, 640, 768);
    linear("edge narrow", c, T, M, 1536, 384);
  }
  // the tile chooser: two workgroups per CU only where there are more workgroups than CUs
  for (int M : {2048, 4600, 9000, 18400, 40000})
    for (int N : {128, 256, 768})
      for (int K : {448, 768, 3072}) linear("edge tile occupancy", c, L, M, K, N);
  // UnivsConfig.linear_rows_per_pass / linear_grid_x / linear_ablate
  const int cfgs[][3] = {{15, 0, 0}, {16, 0, 0}, {64, 0, 0}, {100, 0, 0}, {128, 0, 0}, {192, 0, 0}, {256, 0, 0}, {0, 3, 0}, {0, 4, 0},
                         {0, 5, 0}, {0, 40, 0}, {0, 100000, 0}, {192, 4, 0}, {0, 0, LA_NO_XCD_REMAP}, {0, 0, LA_NO_TILE}, {0, 0, LA_TILE_NSLOT2}, {0, 0, LA_TILE_NSLOT3},
                         {0, 0, LA_TILE_NSLOT4}};
  for (auto& g : cfgs) {
    char l[80];
    snprintf(l, sizeof(l), "config rows_per_pass=%d grid_x=%d ablate=%d", g[0], g[1], g[2]);
    const Ctx o = ctx(256, g[0], g[1], g[2]);
    linear(l, o, R, 96600, 256, 288);
    linear(l, o, T | L, 18400, 1536, 384);
    linear(l, o, T | L, 4600, 768, 2304);
    if (g[2]) linear(l, o, T | L, 4100, 576, 260);
    if (g[2]) linear(l, o, T | L, 18400, 768, 1024);
    dump_conv(l, o, 0, 2, 256, 256, 48, 44);
  }

  // ---- another CU count: no plan hides a literal 256
  gemmset("gemmset T=5 at 64 CUs", ctx(64), 5, 0);
  return 0;
}
