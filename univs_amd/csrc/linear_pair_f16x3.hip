// TWO W-resident Linears on one stream of x in ONE launch (the head of a deformable-encoder layer):
//   problem A:  Ya = x W_a^T + b_a                              (value_proj)
//   problem B:  Yb = (x + add[row % add_rows]) W_b^T + b_b      (the merged sampling-offset / attention-weight projection of `src + pos`)
// both with the column-blocked output of linear_f16x3's EPI_BLOCKED.  Launched apart, the second Linear needs `x + add` as a tensor
// of its own -- a write by its producer and a second read from HBM, 99 MB each at 96 600 x 256 -- and a second W staging, ramp and
// tail.  Here the grid is (row ranges x passes) in linear_f16x3's order (XCD-contiguous, row range major, pass minor), passes
// 0 .. P_a - 1 are A's and P_a .. P_a + P_b - 1 are B's: the passes of a row range are neighbours in one XCD's chunk of the sequence
// (all but the few row ranges that straddle two chunks), x comes from HBM once for both problems, and `add` (one frame's table, the
// same for every frame) is summed onto x in registers as a ring stage is consumed.
//
// ARITHMETIC: each pass is linear_f16x3<RB, RING, true> on its operand -- the same k order, running row scale, two-part split, three
// products smallest first, and epilogue -- and a feature's sum depends on nothing but its own row of W and row of the operand, so each
// problem's output has the bits of univs_linear_blocked_presplit_f32 on the materialised operand (tests/test_encoder_pair_gpu.py).
// The sum x + add is one fp32 add per element, the value the FFN kernel's second output (mlp_f16x3.hip: padd) would have stored.
//
// REGISTERS: a B pass holds `add` next to x, so both of its rings are RING / 2 stages deep: the same registers and the same bytes in
// flight as an A pass's RING stages of x (a k-step of B moves twice the bytes).  With x at the full depth and `add` at half of it, or
// at a quarter, the 96-feature body spills 53 / 16 registers.  The kernel is the two pass bodies behind one uniform branch;
// profiles/encoder_pair_resources_v1.txt has the build's register and scratch figures (no scratch, no spills).
// The k-step -- fragment pipeline, running row scale, three products -- is f16x3_kstep.h, shared with linear_f16x3; the pass around it
// (tile ownership, slab, rings, epilogue) is a second text of that kernel's: as one function both kernels compile into other, longer
// code ("One k-step core").
// What is launched is plan_f16x3_pair (gemm_plan.h).
// MEASURED (profiles/encoder_pair_clip_breakdown_{parent,this}.txt, 96 600 rows): 148 us against the 62 + 88 us of the two launches --
// parity: these projections are bound by the work of their workgroups, all CUs busy either way.  What the launch buys is upstream: the
// FFN kernel without its 99 MB second output (330 -> 299 us per layer), no `src + pos` from tokens_from_nchw, one launch fewer per layer.
#include "common.h"
#include "config.h"
#include "f16x3_kstep.h"
#include "gemm_plan.h"
#include "launchers.h"

namespace univs {

struct PairProblem {
  const u32x4* Wp;       // the pre-split image of presplit_f16x3: [(K / 8) x 2 parts][N] 16-byte units
  const float* winv;     // [N] inverse row scales of the image
  const float* bias;     // [N] or null
  float* Y;              // [M / blk_rows][N / blk_cols][blk_rows][blk_cols]
  int N, rows_per_pass, blk_cols;
};
struct PairArgs {
  const float* X;        // [M, K]
  const float* add;      // [add_rows, K]: B's operand is X[m] + add[m % add_rows]
  int M, K, add_rows, blk_rows, passes_a;
  PairProblem p[2];
};

// One pass: features n0 .. n0 + R - 1 of problem `pr` for the row tiles of row range bx of gx.  AR: ring stages of `add` (0: plain x).
template <int RB, int RING, int AR>
__device__ __forceinline__ void pair_pass(const PairArgs& a, const PairProblem& pr, unsigned bx, unsigned gx, int n0, u32x4* Wsp) {
  const int M = a.M, K = a.K, N = pr.N;
  const int R = min(pr.rows_per_pass, N - n0);                   // a multiple of 4 (host-checked)
  constexpr int Rp = 16 * RB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KS = K >> 5;
  const int j = lane & 15, g = lane >> 4;
  float* bias_lds = reinterpret_cast<float*>(Wsp + (size_t)(K >> 3) * Rp * 2);
  float* winv_lds = bias_lds + R;
  unsigned* tail = reinterpret_cast<unsigned*>(winv_lds + R);    // 64 dwords of zeros

  const int WT = (M + L3_TILE_M - 1) / L3_TILE_M;
  constexpr int NWV = L3_THREADS / 64;
  const int wg0 = (int)((long long)WT * bx / gx), wg1 = (int)((long long)WT * (bx + 1) / gx);
  const int wt0 = wg0 + wave;
  const int ntiles = wt0 < wg1 ? (wg1 - wt0 + NWV - 1) / NWV : 0;

  // byte offsets of the lane's (row, k-group) in x and, for B, in `add`; rows past the end repeat the last row (never stored)
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.X), 0, (int)((long long)M * K * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t ars =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(AR > 0 ? a.add : a.X), 0, (int)((long long)(AR > 0 ? a.add_rows : M) * K * 4), 0x00020000);
  auto tile_voff = [&](int tile, unsigned (&vo)[2], unsigned (&avo)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int m = min((wt0 + tile * NWV) * L3_TILE_M + 16 * c + j, M - 1);
      vo[c] = ((unsigned)m * (unsigned)K + (unsigned)(8 * g)) * 4u;          // < 2^31 (host-checked)
      if constexpr (AR > 0) avo[c] = (((unsigned)m % (unsigned)a.add_rows) * (unsigned)K + (unsigned)(8 * g)) * 4u;
      else avo[c] = 0u;
    }
  };
  // the slab of the split image first and all at once, committed to LDS after the x ring has been requested behind it (linear_f16x3)
  u32x4 wcp[L3_WPT];
  const u32x4* Wp = pr.Wp + n0;
  const int wcp_runs = (K >> 3) * 2;
  const int wcp_rpi = L3_THREADS / R;
  const int wcp_run0 = tid / R;
  const int wcp_rr = tid - wcp_run0 * R;
  const bool wcp_active = wcp_run0 < wcp_rpi;
#pragma unroll
  for (int u = 0; u < L3_WPT; ++u) wcp[u] = Wp[(size_t)min(wcp_run0 + u * wcp_rpi, wcp_runs - 1) * N + wcp_rr];
  __builtin_amdgcn_sched_barrier(0);

  unsigned vo_cur[2], vo_next[2], avo_cur[2], avo_next[2];
  tile_voff(0, vo_cur, avo_cur);
  tile_voff(min(1, max(ntiles, 1) - 1), vo_next, avo_next);
  f32x4 raw[RING][2][2];                                         // [stage][column tile][16-byte half]
  f32x4 addr[AR > 0 ? AR : 1][2][2];
  auto load_rows = [&](f32x4 (&buf)[2][2], const __amdgpu_buffer_rsrc_t rs, const unsigned (&vo)[2], int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      buf[c][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo[c], ks * 128, 0));
      buf[c][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo[c] + 16u, ks * 128, 0));
    }
  };
#pragma unroll
  for (int u = 0; u < RING; ++u) {
    load_rows(raw[u], xrs, vo_cur, u);                           // RING <= KS
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (AR > 0) {
#pragma unroll
    for (int u = 0; u < AR; ++u) {
      load_rows(addr[u], ars, avo_cur, u);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  for (int r = tid; r < R; r += L3_THREADS) {
    bias_lds[r] = pr.bias ? pr.bias[n0 + r] : 0.f;
    winv_lds[r] = pr.winv[n0 + r];
  }
  for (int i = tid; i < 64; i += L3_THREADS) tail[i] = 0u;
#pragma unroll
  for (int u = 0; u < L3_WPT; ++u)
    if (wcp_active && wcp_run0 + u * wcp_rpi < wcp_runs) Wsp[(size_t)(wcp_run0 + u * wcp_rpi) * Rp + wcp_rr] = wcp[u];
  __syncthreads();   // the only barrier
  if (ntiles == 0) return;

  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(pr.Y, 0, (int)((long long)M * N * 4), 0x00020000);
  const int blk_rows = a.blk_rows, blk_cols = pr.blk_cols;

  f32x4 acc[RB][2];
  int eset[2];                                                    // exponent the running scale of my two rows was set for
  float sx[2], sx_inv[2];

  auto epilogue = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int m = (wt0 + tile * NWV) * L3_TILE_M + 16 * c + j;
      const unsigned b = (unsigned)m / (unsigned)blk_rows;
      const unsigned rowpart = b * (unsigned)blk_rows * (unsigned)N + ((unsigned)m - b * (unsigned)blk_rows) * (unsigned)blk_cols;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const int f = rb * 16 + 4 * g;
        const int fc = min(f, R - 4);
        const f32x4 wi = *reinterpret_cast<const f32x4*>(winv_lds + fc);
        const f32x4 bi = *reinterpret_cast<const f32x4*>(bias_lds + fc);
        const f32x4 v = (acc[rb][c] * sx_inv[c]) * wi + bi;        // two exact unscalings, then the bias
        const unsigned fg = (unsigned)(n0 + f);
        const unsigned cb = fg / (unsigned)blk_cols;
        const unsigned off = (rowpart + cb * (unsigned)blk_rows * (unsigned)blk_cols + (fg - cb * (unsigned)blk_cols)) * 4u;
        // out of range: the store is dropped
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yrs, (m < M && f < R) ? off : 0xFFFFFFF0u, 0, 0);
      }
    }
  };

  using KS_ = KStep<RB>;                                         // the A-fragment pipeline of f16x3_kstep.h
  constexpr int NB = KS_::NB;
  typename KS_::Batch afr[2];
  const unsigned a_lane = KS_::lane(g, j);
  auto read_batch = l3_batch_reader<RB>();
  auto group = [&](int ks0, bool last_group) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < RING; ++u) {
      const int ks = ks0 + u;
      if constexpr (AR > 0) {                                     // B's operand, formed in the ring stage: one fp32 add per element
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          raw[u][c][0] = raw[u][c][0] + addr[u % AR][c][0];
          raw[u][c][1] = raw[u][c][1] + addr[u % AR][c][1];
        }
      }
      int enew[2];                                                // the running row scale (f16x3_kstep.h)
      if (__builtin_amdgcn_ballot_w64(l3_row_scale_need(raw[u], eset, enew)) != 0) l3_row_scale_lower(enew, acc, eset, sx, sx_inv);   // rare
      float s0 = sx[0], s1 = sx[1];
      asm volatile("" : "+v"(s0), "+v"(s1) : : "memory");      // pins the consumption of ring stage u here
      f16x8 bh[2], bm[2];
      l3_split8(raw[u][0][0], raw[u][0][1], s0, bh[0], bm[0]);
      l3_split8(raw[u][1][0], raw[u][1][1], s1, bh[1], bm[1]);
      __builtin_amdgcn_sched_barrier(0);
      {                                                           // refill the stages just consumed
        const int ksn = last_group ? u : ks + RING;
        if (last_group) load_rows(raw[u], xrs, vo_next, ksn);
        else load_rows(raw[u], xrs, vo_cur, ksn);
        if constexpr (AR > 0) {                                   // `add` runs AR k-steps ahead: into the next tile from u = RING - AR
          const bool wrap = last_group && (u + AR >= RING);
          const int ksa = wrap ? u + AR - RING : ks + AR;
          if (wrap) load_rows(addr[u % AR], ars, avo_next, ksa);
          else load_rows(addr[u % AR], ars, avo_cur, ksa);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      const int ks_next = (ks + 1 == KS) ? 0 : ks + 1;
      l3_static_for<0, NB>([&](auto bc) __attribute__((always_inline)) {
        constexpr int b = decltype(bc)::value;
        l3_wait_batch(afr[b & 1]);
        if constexpr (b + 1 < NB) read_batch(afr[(b + 1) & 1], a_lane + (unsigned)ks * KS_::kstep, std::integral_constant<int, b + 1>{});
        else read_batch(afr[0], a_lane + (unsigned)ks_next * KS_::kstep, std::integral_constant<int, 0>{});
        __builtin_amdgcn_sched_barrier(0);
        l3_mfma_batch<RB, b>(afr[b & 1], bh, bm, acc);
        __builtin_amdgcn_sched_barrier(0);
      });
    }
  };

  read_batch(afr[0], a_lane, std::integral_constant<int, 0>{});                          // batch 0 of the first k-step

#pragma unroll 1
  for (int tile = 0; tile < ntiles; ++tile) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb][0] = acc[rb][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    l3_row_scale_reset(eset, sx, sx_inv);
#pragma unroll 1
    for (int ks0 = 0; ks0 < KS; ks0 += RING) group(ks0, ks0 + RING >= KS);
    epilogue(tile);
    vo_cur[0] = vo_next[0];
    vo_cur[1] = vo_next[1];
    avo_cur[0] = avo_next[0];
    avo_cur[1] = avo_next[1];
    tile_voff(min(tile + 2, ntiles - 1), vo_next, avo_next);
  }
}

template <int RBA, int RBB, int RING>
__global__ __launch_bounds__(L3_THREADS, 1) void linear_pair_f16x3(const PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) u32x4 Wsp[];
  // (row range, pass) of this workgroup: every XCD a contiguous chunk of the sequence, row range major, pass minor (linear_f16x3)
  const unsigned lw = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
  const unsigned bx = lw / gridDim.y;
  const int by = __builtin_amdgcn_readfirstlane((int)(lw - bx * gridDim.y));
  if (by < a.passes_a)
    pair_pass<RBA, RING, 0>(a, a.p[0], bx, gridDim.x, by * a.p[0].rows_per_pass, Wsp);
  else
    pair_pass<RBB, RING / 2, RING / 2>(a, a.p[1], bx, gridDim.x, (by - a.passes_a) * a.p[1].rows_per_pass, Wsp);
}

// returns 1 if launched, 0 if not covered, < 0 on error
int linear_pair_f16x3_f32(const float* x, const float* add, long long add_rows, const void* wp_a, const float* winv_a, const float* bias_a,
                          int N_a, int blk_cols_a, float* y_a, const void* wp_b, const float* winv_b, const float* bias_b, int N_b,
                          int blk_cols_b, float* y_b, long long M, int K, long long blk_rows, hipStream_t st) {
  if (!pair_covered(M, N_a, N_b, K, add_rows, blk_rows, blk_cols_a, blk_cols_b) ||
      !aligned16(x, add, static_cast<const float*>(wp_a), winv_a, bias_a, y_a, static_cast<const float*>(wp_b), winv_b, bias_b, y_b))
    return 0;
  const PairPlan p = plan_f16x3_pair(M, N_a, N_b, K, cu_count());
  if (!p.covered || p.RB[0] != 8 || p.RB[1] != 6 || p.ring != 4) return 0;   // the one instantiation: passes of 128 and of 96 features
  PairArgs a;
  a.X = x; a.add = add; a.M = (int)M; a.K = K; a.add_rows = (int)add_rows; a.blk_rows = (int)blk_rows; a.passes_a = (int)p.passes[0];
  a.p[0] = PairProblem{static_cast<const u32x4*>(wp_a), winv_a, bias_a, y_a, N_a, p.rows_per_pass[0], blk_cols_a};
  a.p[1] = PairProblem{static_cast<const u32x4*>(wp_b), winv_b, bias_b, y_b, N_b, p.rows_per_pass[1], blk_cols_b};
  dim3 grid(p.gx, p.passes[0] + p.passes[1]), block(L3_THREADS);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&linear_pair_f16x3<8, 6, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
  hipLaunchKernelGGL((linear_pair_f16x3<8, 6, 4>), grid, block, p.lds, st, a);
  const int rc = check_launch("linear_pair_f16x3_f32");
  return rc == UNIVS_OK ? 1 : rc;
}

}  // namespace univs
