// y[M, N] = x[M, K] * W[N, K]^T + bias[N]  (nn.Linear, fp32) on the fp16 matrix cores of gfx950 in THREE passes.
//
// linear_split.hip multiplies fp32 operands as three bf16 parts each (8 + 8 + 8 mantissa bits) and keeps six of the nine
// part products.  bf16 was chosen there for its exponent range; fp16 parts carry 11 bits each, so TWO parts hold 22 - 23
// bits and THREE products (h h', h m', m h') do the work of six -- if the operands are first brought into fp16's range:
//   * every row of x and every row of W is scaled by a power of two that puts its largest magnitude in [2^14, 2^15)
//     (exact; the product is unscaled by the two inverse powers in the epilogue, exact again).  The row maximum of W is
//     taken while the workgroup stages its slab (LDS atomic max on the magnitude bits).  x is read ONCE: its rows carry a
//     RUNNING scale, set from the first k-step and lowered -- with an exact rescaling of the row's accumulators -- when a
//     later k-step would leave the range (see the kernel; a separate maximum pass cost 25 - 40 % of the kernel, a
//     look-ahead register ring no less: these Linears run close to the HBM time of x and y);
//   * x' = h + m + r with h = fp16(x') and m = fp16(x' - h), both round-to-nearest: |r| <= 2^-23 |x'| for elements within
//     2^-16 of their row's maximum, and 2^-25 absolute (scaled units, i.e. 2^-39 of the row maximum) below that (m becomes
//     subnormal);  dropped: m m' (<= 2^-24) and the representation errors (<= 2^-23 each): <= 2^-21.7 per product, against
//     3 x 2^-24 = 2^-22.4 for the six-term bf16 split.  Both are below the rounding error of an fp32 FMA chain over K >= 96
//     terms: measured against fp64 on the operator's shapes the result is as close as ATen's own fp32 GEMM or closer
//     (tests/test_ops_gpu.py: test_linear_split_matches_torch runs for both splits);
//   * products accumulate in fp32 on v_mfma_f32_16x16x32_f16; Inf / NaN inputs poison their own row only (as in a GEMM):
//     the row maximum ignores NaN (maxNum) and an infinite maximum scales the finite elements to ~0, the row's results
//     are Inf / NaN either way.
// Everything else IN THE KERNEL is the organisation of linear_bf16x6 (linear_split.hip): W slab resident in LDS in A-fragment order
// (4 bytes per element instead of 6: 128 output features of K = 256 per pass, N = 256 in two passes instead of three),
// x streamed through a register ring, D[i = feature][j = row] so that a lane stores four consecutive features of one row,
// epilogues ReLU / GELU / residual / column-blocked output.
// What is launched -- coverage, passes, row ranges, LDS bytes -- is plan_f16x3_resident (gemm_plan.h), shared with linear_split.hip.
#include "common.h"
#include "config.h"
#include "f16x3_kstep.h"
#include "gemm_plan.h"
#include "launchers.h"

#include <algorithm>
#include <cstdlib>

namespace univs {

#ifdef UNIVS_TRACE_GEMM
UNIVS_GT_DECL(g_l3_trace);
#endif
enum { L3_EPI_NONE = EPI_NONE, L3_EPI_RELU = EPI_RELU, L3_EPI_GELU = EPI_GELU, L3_EPI_RESIDUAL = EPI_RESIDUAL, L3_EPI_BLOCKED = EPI_BLOCKED };

// LDS: Wsp [K/32][4 k-groups][2 parts][16 RB features] 16 B | bias[R] | winv[R] | zero tail (16 x 16 B) | wmax[R]
// PRE: W is the pre-split image of presplit_f16x3 (gemm_f16x3_stream.hip: [(K / 8) x 2 parts][N] 16-byte units, `winv_g` its
// inverse row scales) and staging the slab is a COPY.  Splitting the slab inside every workgroup (row maxima by LDS atomics,
// then scale + split: two dependent sweeps over the slab) measured 28 - 32 k clocks = 13 - 15 us at the head of EVERY launch --
// a quarter of an 18 400-row Swin stage-3 Linear, 30 % of a 96 600-row encoder projection (profiles/r05_gemm_phase_trace_v1.txt).
template <int RB, int RING, bool PRE>   // RING: register stages of x (K / 32 is a multiple)
__global__ __launch_bounds__(L3_THREADS, 1) void linear_f16x3(const float* __restrict__ X,      // [M, K]
                                                               const float* __restrict__ W,      // [N, K] (PRE: the split image)
                                                               const float* __restrict__ bias,   // [N] or null
                                                               const float* __restrict__ Res,    // [M, N] (epi == RESIDUAL)
                                                               float* __restrict__ Y,            // [M, N]
                                                               int M, int N, int K, int rows_per_pass, int epi, int blk_rows,
                                                               int blk_cols, int ablate, const float* __restrict__ winv_g) {
  extern __shared__ __attribute__((aligned(16))) u32x4 Wsp[];
  [[maybe_unused]] const int gts = UNIVS_GT_SLOT();
  UNIVS_GT(g_l3_trace, gts, 0);
  UNIVS_GT_REAL(g_l3_trace, gts, 62);
  // (row range, pass) of this workgroup.  Workgroups go to the 8 XCDs round-robin by linear id; the remap gives every XCD a CONTIGUOUS
  // chunk of the sequence (row range major, pass minor): the passes of a row range -- which stream the same rows of x -- run on ONE XCD
  // and meet in its L2, whatever the grid extents (with 12 passes over 21 row ranges every XCD used to fetch nearly all of x itself).
  unsigned bx = blockIdx.x, by = blockIdx.y;
  if (ablate != LA_NO_XCD_REMAP && gridDim.y > 1) {
    const unsigned lw = xcd_remap(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    bx = lw / gridDim.y;
    by = lw - bx * gridDim.y;
  }
  const int n0 = by * rows_per_pass;
  const int R = min(rows_per_pass, N - n0);                      // a multiple of 4 (host-checked)
  constexpr int Rp = 16 * RB;                                    // rows of the LDS image (rows >= R are never written: their
                                                                 // products only reach features that are never stored)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int KS = K >> 5;
  const int j = lane & 15, g = lane >> 4;
  float* bias_lds = reinterpret_cast<float*>(Wsp + (size_t)(K >> 3) * Rp * 2);
  float* winv_lds = bias_lds + R;
  unsigned* tail = reinterpret_cast<unsigned*>(winv_lds + R);    // 64 dwords of zeros
  unsigned* wmax_lds = tail + 64;

  // ---- this wave's row tiles: the workgroup owns a contiguous run, its waves take tiles round-robin
  const int WT = (M + L3_TILE_M - 1) / L3_TILE_M;
  constexpr int NWV = L3_THREADS / 64;
  const int wg0 = (int)((long long)WT * bx / gridDim.x), wg1 = (int)((long long)WT * (bx + 1) / gridDim.x);
  const int wt0 = wg0 + wave;
  const int ntiles = wt0 < wg1 ? (wg1 - wt0 + NWV - 1) / NWV : 0;

  // x through buffer loads: the lane's byte offset (row, k-group) is computed once per tile, the k-step is the scalar
  // offset -- no vector arithmetic per load.  Rows past the end repeat the last row (their results are not stored).
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(X), 0, (int)((long long)M * K * 4), 0x00020000);
  auto tile_voff = [&](int tile, unsigned (&vo)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int m = min((wt0 + tile * NWV) * L3_TILE_M + 16 * c + j, M - 1);
      vo[c] = ((unsigned)m * (unsigned)K + (unsigned)(8 * g)) * 4u;          // < 2^31 (host-checked)
    }
  };
  // PRE: this pass's slab of the split image, requested FIRST and all at once (<= L3_WPT 16-byte units per thread), committed to LDS
  // after the x ring has been requested behind it: vector memory returns in order, so the wait for the slab does not wait for x
  // (requested behind x, each sweep of the copy waited for the first tiles' rows to arrive from HBM: 14 - 17 k clocks instead of ~4 k).
  // run = (k-group of 8, part): R consecutive units of the image, N units apart; R threads per run, 512 / R runs per sweep.
  [[maybe_unused]] u32x4 wcp[L3_WPT];
  [[maybe_unused]] int wcp_runs = 0, wcp_rpi = 1, wcp_run0 = 0, wcp_rr = 0;
  [[maybe_unused]] bool wcp_active = false;
  if constexpr (PRE) {
    const u32x4* Wp = reinterpret_cast<const u32x4*>(W) + n0;
    wcp_runs = (K >> 3) * 2;
    wcp_rpi = L3_THREADS / R;
    wcp_run0 = tid / R;
    wcp_rr = tid - wcp_run0 * R;
    wcp_active = wcp_run0 < wcp_rpi;
#pragma unroll
    for (int u = 0; u < L3_WPT; ++u) wcp[u] = Wp[(size_t)min(wcp_run0 + u * wcp_rpi, wcp_runs - 1) * N + wcp_rr];
    __builtin_amdgcn_sched_barrier(0);
  }
  unsigned vo_cur[2], vo_next[2];
  tile_voff(0, vo_cur);
  tile_voff(min(1, max(ntiles, 1) - 1), vo_next);
  f32x4 raw[RING][2][2];                                         // [stage][column tile][16-byte half]
  auto load_x = [&](f32x4 (&buf)[2][2], const unsigned (&vo)[2], int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      buf[c][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, vo[c], ks * 128, 0));
      buf[c][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, vo[c] + 16u, ks * 128, 0));
    }
  };
#pragma unroll
  for (int u = 0; u < RING; ++u) {
    load_x(raw[u], vo_cur, u);                                   // RING <= KS
    __builtin_amdgcn_sched_barrier(0);
  }

  UNIVS_GT(g_l3_trace, gts, 1);
  // ---- this pass's rows of W -> LDS (fragment order), two sweeps: row maxima, then scale + split.  Work item = 8
  // consecutive k of one row; consecutive threads take consecutive ROWS (conflict-free 16-byte LDS writes; the reads of W
  // are 32-byte pieces of different rows, all L2 hits after the first workgroup)
  const float* Wsrc = W + (size_t)n0 * K;
  const int kch = K >> 3;
  for (int r = tid; r < R; r += L3_THREADS) {
    wmax_lds[r] = 0u;
    bias_lds[r] = bias ? bias[n0 + r] : 0.f;
    if constexpr (PRE) winv_lds[r] = winv_g[n0 + r];
  }
  for (int i = tid; i < 64; i += L3_THREADS) tail[i] = 0u;
  if constexpr (PRE) {                                             // commit the slab requested at the top of the kernel
#pragma unroll
    for (int u = 0; u < L3_WPT; ++u)
      if (wcp_active && wcp_run0 + u * wcp_rpi < wcp_runs) Wsp[(size_t)(wcp_run0 + u * wcp_rpi) * Rp + wcp_rr] = wcp[u];
  }
  if constexpr (!PRE) {
    __syncthreads();
    for (int idx = tid; idx < R * kch; idx += L3_THREADS) {
      const int kc = idx / R, r = idx - kc * R;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(Wsrc + (size_t)r * K + kc * 8);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(Wsrc + (size_t)r * K + kc * 8 + 4);
      atomicMax(&wmax_lds[r], l3_absmax8(x0, x1));
    }
    __syncthreads();
    for (int idx = tid; idx < R * kch; idx += L3_THREADS) {
      const int kc = idx / R, r = idx - kc * R;
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(Wsrc + (size_t)r * K + kc * 8);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(Wsrc + (size_t)r * K + kc * 8 + 4);
      float s, inv;
      l3_scale(wmax_lds[r], 14, s, inv);
      f16x8 h, m;
      l3_split8(x0, x1, s, h, m);
      u32x4* dst = Wsp + (size_t)(kc * 2) * Rp + r;                // kc = ks * 4 + k-group
      dst[0] = __builtin_bit_cast(u32x4, h);
      dst[Rp] = __builtin_bit_cast(u32x4, m);
      if (kc == 0) winv_lds[r] = inv;
    }
  }
  __syncthreads();   // the only barrier of the main part
  UNIVS_GT(g_l3_trace, gts, 2);
  UNIVS_GT_VAL(g_l3_trace, gts, 63, ntiles);
  if (ntiles == 0) return;

  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(Y, 0, (int)((long long)M * N * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rrs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(epi == L3_EPI_RESIDUAL ? Res : X), 0, (int)((long long)M * N * 4), 0x00020000);

  f32x4 acc[RB][2];
  // the running scale of my two rows (f16x3_kstep.h)
  int eset[2];                                                    // exponent the scale of my two rows was set for
  float sx[2], sx_inv[2];

  auto epilogue = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int m = (wt0 + tile * NWV) * L3_TILE_M + 16 * c + j;
      unsigned rowpart = 0;
      if (epi == L3_EPI_BLOCKED) {
        const unsigned b = (unsigned)m / (unsigned)blk_rows;
        rowpart = b * (unsigned)blk_rows * (unsigned)N + ((unsigned)m - b * (unsigned)blk_rows) * (unsigned)blk_cols;
      }
      auto out_off = [&](int rb) __attribute__((always_inline)) -> unsigned {
        const int f = rb * 16 + 4 * g;
        unsigned off = ((unsigned)m * (unsigned)N + (unsigned)(n0 + f)) * 4u;
        if (epi == L3_EPI_BLOCKED) {
          const unsigned fg = (unsigned)(n0 + f);
          const unsigned cb = fg / (unsigned)blk_cols;
          off = (rowpart + cb * (unsigned)blk_rows * (unsigned)blk_cols + (fg - cb * (unsigned)blk_cols)) * 4u;
        }
        return (m < M && f < R) ? off : 0xFFFFFFF0u;             // out of range: loads return 0, stores are dropped
      };
      // the residual values of this column tile, requested together: a load inside the per-block loop is compiled into load / wait /
      // store -- one memory latency per block, RB per column tile (enc_output_proj + residual: 91 us against 62 us without)
      constexpr int RBAT = RB > 4 ? (RB + 1) / 2 : RB;           // (in two halves at RB > 4: registers)
      f32x4 resv[RBAT];
      auto load_res = [&](int rb0) __attribute__((always_inline)) {
        if (epi == L3_EPI_RESIDUAL) {
#pragma unroll
          for (int q = 0; q < RBAT; ++q)
            resv[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rrs, out_off(min(rb0 + q, RB - 1)), 0, 0));
        } else {
#pragma unroll
          for (int q = 0; q < RBAT; ++q) resv[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      };
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        if (rb % RBAT == 0) load_res(rb);
        const int f = rb * 16 + 4 * g;
        const int fc = min(f, R - 4);
        const f32x4 wi = *reinterpret_cast<const f32x4*>(winv_lds + fc);
        const f32x4 bi = *reinterpret_cast<const f32x4*>(bias_lds + fc);
        f32x4 v = (acc[rb][c] * sx_inv[c]) * wi + bi;              // two exact unscalings, then the bias
        const unsigned offc = out_off(rb);
        if (epi == L3_EPI_RELU) v = __builtin_elementwise_maximum(v, (f32x4){0.f, 0.f, 0.f, 0.f})   /* NaN-propagating, as torch.relu */;
        if (epi == L3_EPI_GELU) {   // x * 0.5 * (1 + erf(x / sqrt 2)): nn.GELU() (approximate = 'none')
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = l3_gelu(v[e]);
        }
        if (epi == L3_EPI_RESIDUAL) v += resv[rb % RBAT];
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yrs, offc, 0, 0);
      }
    }
  };

  // A fragments (W parts) from LDS, one batch ahead of the MFMAs that use them (f16x3_kstep.h)
  using KS_ = KStep<RB>;
  constexpr int NB = KS_::NB;
  typename KS_::Batch afr[2];                                    // [buffer]: the batch in use and the one being read
  const unsigned a_lane = KS_::lane(g, j);
  auto read_batch = l3_batch_reader<RB>();
  auto group = [&](int ks0, bool last_group) __attribute__((always_inline)) {
    unsigned vo_ref[2];                                           // rows of the k-steps requested in this group
#pragma unroll
    for (int c = 0; c < 2; ++c) vo_ref[c] = last_group ? vo_next[c] : vo_cur[c];
#pragma unroll
    for (int u = 0; u < RING; ++u) {
      const int ks = ks0 + u;
      int enew[2];                                                // the running row scale
      if (__builtin_amdgcn_ballot_w64(l3_row_scale_need(raw[u], eset, enew)) != 0 && ablate != LA_SCALE_FROZEN) l3_row_scale_lower(enew, acc, eset, sx, sx_inv);   // rare
      float s0 = sx[0], s1 = sx[1];
      asm volatile("" : "+v"(s0), "+v"(s1) : : "memory");      // pins the consumption of ring stage u here
      f16x8 bh[2], bm[2];
      l3_split8(raw[u][0][0], raw[u][0][1], s0, bh[0], bm[0]);
      l3_split8(raw[u][1][0], raw[u][1][1], s1, bh[1], bm[1]);
      __builtin_amdgcn_sched_barrier(0);
      {                                                           // refill the stage just consumed (RING steps ahead)
        const int ksn = last_group ? u : ks + RING;
        load_x(raw[u], vo_ref, ksn);
      }
      __builtin_amdgcn_sched_barrier(0);
      const int ks_next = (ks + 1 == KS) ? 0 : ks + 1;           // the next k-step's first batch (W is the same for every tile)
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
    l3_row_scale_reset(eset, sx, sx_inv, ablate == LA_SCALE_FROZEN);
#pragma unroll 1
    for (int ks0 = 0; ks0 < KS; ks0 += RING) group(ks0, ks0 + RING >= KS);
    UNIVS_GT(g_l3_trace, gts, 3 + 2 * tile);
    epilogue(tile);
    UNIVS_GT(g_l3_trace, gts, 4 + 2 * tile);
    vo_cur[0] = vo_next[0];
    vo_cur[1] = vo_next[1];
    tile_voff(min(tile + 2, ntiles - 1), vo_next);
  }
  UNIVS_GT_REAL(g_l3_trace, gts, 61);
}

// The three-product launch of linear_split_f32 (linear_split.hip), which has run the shared predicates and read the CU count:
// returns 1 if launched, 0 if not covered, < 0 on error.
// `winv` != nullptr: `w` is the pre-split image (univs_presplit_weights_f32, mode 0) and `winv` its inverse row scales
int linear_f16x3_f32(const float* x, const float* w, const float* bias, const float* residual, float* y, long long M, int N,
                     int K, int epi, hipStream_t st, int blk_rows, int blk_cols, const float* winv, int n_cu) {
  const UnivsConfig cfg_ = config();
  const ResidentPlan p = plan_f16x3_resident(M, N, K, winv != nullptr, n_cu, cfg_);
  if (!p.covered || (reinterpret_cast<uintptr_t>(winv) & 3)) return 0;
  const int RB = p.RB, ring = p.ring, rows = p.rows_per_pass;
  const size_t lds = p.lds;
  dim3 grid(p.gx, p.passes), block(L3_THREADS);
#define UNIVS_L3(rb, rg, pre)                                                                                             \
  do {                                                                                                               \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&linear_f16x3<rb, rg, pre>),                                  \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                 \
    hipLaunchKernelGGL((linear_f16x3<rb, rg, pre>), grid, block, lds, st, x, w, bias, residual, y, (int)M, N, K, rows, epi, \
                       blk_rows, blk_cols, cfg_.linear_ablate, winv);                                                                              \
  } while (0)
#define UNIVS_L3_RB(rb)                                    \
  case rb:                                                 \
    if (winv) {                                            \
      if (ring == 4) { UNIVS_L3(rb, 4, true); }            \
      else { UNIVS_L3(rb, 3, true); }                      \
    } else {                                               \
      if (ring == 4) { UNIVS_L3(rb, 4, false); }           \
      else { UNIVS_L3(rb, 3, false); }                     \
    }                                                      \
    break
  switch (RB) {
    UNIVS_L3_RB(1);
    UNIVS_L3_RB(2);
    UNIVS_L3_RB(3);
    UNIVS_L3_RB(4);
    UNIVS_L3_RB(5);
    UNIVS_L3_RB(6);
    UNIVS_L3_RB(7);
    default: UNIVS_L3_RB(8);
  }
#undef UNIVS_L3_RB
#undef UNIVS_L3
  const int rc = check_launch("linear_f16x3_f32");
  return rc == UNIVS_OK ? 1 : rc;
}

}  // namespace univs

#ifdef UNIVS_TRACE_GEMM
extern "C" int univs_debug_gemm_trace_linear(unsigned long long* out, int clear) {
  if (clear) {
    static unsigned long long zeros[UNIVS_GT_SLOTS * UNIVS_GT_STAMPS] = {};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(univs::g_l3_trace), zeros, sizeof(zeros));
  }
  (void)hipDeviceSynchronize();
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(univs::g_l3_trace), sizeof(unsigned long long) * UNIVS_GT_SLOTS * UNIVS_GT_STAMPS);
}
#endif
