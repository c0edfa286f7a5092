// The two projections at the head of a deformable-encoder layer (linear_pair_f16x3.hip: A = value_proj on x, B = the merged sampling
// projection on x + add[row % add_rows], both column-blocked) with the operand RESIDENT and the weights STREAMED -- the organisation of
// the FFN kernel's first product (mlp_f16x3.hip) instead of the W-resident passes of linear_pair_f16x3.
//
// WHY: the pass kernel walks x once per pass (2 of A, 3 of B) and every pass repeats the vector prologue of a k-step -- row maximum,
// running scale, the two-instruction split -- on the same elements: five times per element of x, and in this family vector work between
// a wave's matrix instructions adds to its time.  Here a workgroup (8 waves) is persistent over groups of 128 rows and a wave owns 16 rows:
//   * per row group the wave reads its 16 x 256 tile of x ONCE, and `add` beside it, and keeps the two fp16 parts of every k-step of
//     BOTH operands in registers (2 x 64), each split with the scale the running-scale rule of f16x3_kstep.h gives that k-step, together
//     with the rule's SCHEDULE: at which k-steps the scale of the row was lowered, and by which power of two;
//   * the split images of W_a, then W_b, stream through LDS in chunks of 32 features (64 runs of 512 B = 32 KB), global -> LDS by DMA,
//     in a ring of four images, the chunk three ahead requested during the current one (a chunk is ~1.5k clocks of matrix
//     instructions per SIMD, less than a loaded L2's latency: with two images the barrier waited for the stream), one barrier per
//     chunk: 8 chunks of A, 9 of B per row group;
//   * a chunk's k loop replays the schedule: where the scale was lowered at k-step t, the chunk's accumulators are multiplied by the
//     same exact power of two before the k-step's three products (l3_mfma3_pair: f16x3.h's order).
// ARITHMETIC: a feature's sum depends on its row of W, its row of the operand and that row's sequence of scales only, and all three are
// those of linear_f16x3<.., true> -- so each output has the bits of linear_pair_f16x3 and of univs_linear_blocked_presplit_f32 on the
// materialised operand (tests/test_encoder_pair_xres_gpu.py).  The lowering is decided wave-wide by ballot there (32 rows) and here
// (16 rows); a row that does not need it is multiplied by 2^0 and keeps its scale, so the vote's width does not enter the result.
// STORES: a chunk's 32 features of 16 rows leave as two 16-byte stores per lane, issued in the NEXT chunk behind its DMA requests: the
// counted wait for a chunk's pieces in front of its barrier then reaches back only to stores three chunks old (see the loop).
// Stream pieces, fragment reads (two batches ahead) and counted lgkmcnt waits are f16x3_wstream.h's; the schedule below is this kernel's.
// Covered: pair_xres_plan.h.  profiles/encoder_xres_resources_v1.txt has the build's register, LDS and scratch figures.
// MEASURED (profiles/encoder_xres_clip_breakdown_{parent,this}.txt, 96 600 rows): 120.7 us against the pass kernel's 148.5 on the same
// box.  Its parts add rather than overlap (profiles/encoder_xres_ablation_v1.txt): stores 20 us, matrix instructions 28, LDS reads 19,
// weight stream 12, and 56 us for what is left without them -- mostly the tile build, which nothing runs beside.
#include "common.h"
#include "config.h"
#include "f16x3_wstream.h"
#include "pair_xres_plan.h"

namespace univs {

struct XresProblem {
  const u32x4* Wp;       // the pre-split image of presplit_f16x3: [(K / 8) x 2 parts][N] 16-byte units
  const float* winv;     // [N] inverse row scales of the image
  const float* bias;     // [N] or null
  float* Y;              // [M / blk_rows][N / blk_cols][blk_rows][blk_cols]
  int N, blk_cols;
};
struct XresArgs {
  const float* X;        // [M, K]
  const float* add;      // [add_rows, K]: B's operand is X[m] + add[m % add_rows]
  int M, add_rows, blk_rows, nwg;
  XresProblem p[2];
};

// The running row scale of f16x3_kstep.h for ONE row per lane (l3_row_scale_need / l3_row_scale_lower hold two), with the accumulators'
// rescaling recorded instead of applied: `sched` byte t = the biased exponent of the ratio 2^(old - new) of k-step t, `mask` bit t = some
// row of the wave was lowered at k-step t (wave-uniform).
struct PxScale {
  int eset;
  float sx, sx_inv;
  unsigned sched[2], mask;
};
template <int T>
__device__ __forceinline__ void px_scale_step(const f32x4 v0, const f32x4 v1, PxScale& s) {
  const unsigned mk = l3_row_max(l3_absmax8(v0, v1));
  const int enew = l3_scale_exp(mk);
  const bool mine = l3_scale_stale(enew, s.eset);
  if (__builtin_amdgcn_ballot_w64(mine) != 0) {                               // rare after the first k-step
    const int en = mine ? enew : s.eset;
    const unsigned rexp = l3_scale_ratio_exp(s.eset, en);                     // ratio 2^(old - new) <= 1
    s.sched[T >> 2] |= rexp << (8 * (T & 3));
    s.mask |= 1u << T;
    s.eset = en;
    s.sx = l3_scale_of(en);
    s.sx_inv = l3_scale_inv_of(en);
  }
}

template <int KS>
__global__ __launch_bounds__(PX_THREADS) void linear_pair_xres(const XresArgs a) {
  extern __shared__ __attribute__((aligned(16))) u32x4 Lds[];
  constexpr int K = 32 * KS;
  constexpr int CHU = KS * 4 * 2 * PX_CHUNK;                     // 16-byte units of a chunk image
  constexpr int UPT = CHU / PX_THREADS;                          // ... per thread: one DMA piece per wave each
  static_assert(CHU % PX_THREADS == 0 && UPT < KS && KS >= 3 && PX_IMAGES >= 3, "chunk geometry");
  const int M = a.M;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int ngroups = (M + PX_ROWS - 1) / PX_ROWS;
  if ((int)blockIdx.x >= ngroups) return;
  const int NA = a.p[0].N, NB = a.p[1].N;
  float* bias_a = reinterpret_cast<float*>(Lds + PX_IMAGES * CHU);
  float* winv_a = bias_a + NA;
  float* bias_b = winv_a + NA;
  float* winv_b = bias_b + NB;
  for (int r = tid; r < NA; r += PX_THREADS) {
    bias_a[r] = a.p[0].bias ? a.p[0].bias[r] : 0.f;
    winv_a[r] = a.p[0].winv[r];
  }
  for (int r = tid; r < NB; r += PX_THREADS) {
    bias_b[r] = a.p[1].bias ? a.p[1].bias[r] : 0.f;
    winv_b[r] = a.p[1].winv[r];
  }

  // ---- weight stream: unit i = tid + PX_THREADS v of a chunk image is unit ((i >> 5) N + 32 c + (i & 31)) of the split image
  const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)Lds);
  // piece v of chunk c: base Wp + 16 v N + 32 c (uniform), lane offset (tid >> 5) N + (tid & 31) units
  auto w_base = [&](const XresProblem& pr, int c, int v) __attribute__((always_inline)) -> const u32x4* {
    return pr.Wp + ((size_t)(PX_THREADS / 32) * v * pr.N + PX_CHUNK * c);
  };
  auto w_voff = [&](const XresProblem& pr) __attribute__((always_inline)) -> unsigned {
    return ((unsigned)(tid >> 5) * (unsigned)pr.N + (unsigned)(tid & 31)) * 16u;
  };
#pragma unroll
  for (int v = 0; v < (PX_IMAGES - 1) * UPT; ++v)                // A's first chunks -> images 0 .. PX_IMAGES - 2 (N_a: host-checked)
    l3_glds16(w_base(a.p[0], v / UPT, v % UPT), w_voff(a.p[0]), lds_base + (unsigned)(((v / UPT) * CHU + PX_THREADS * (v % UPT) + 64 * wave) * 16));

  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.X), 0, (int)((long long)M * K * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.add), 0, (int)((long long)a.add_rows * K * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs_a = __builtin_amdgcn_make_buffer_rsrc(a.p[0].Y, 0, (int)((long long)M * NA * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs_b = __builtin_amdgcn_make_buffer_rsrc(a.p[1].Y, 0, (int)((long long)M * NB * 4), 0x00020000);

  u32x4 afr[3][2][2];                                            // [ring][block][part]
  // batch T = k-step T of a chunk image at lane address `addr`: the k-step, block and part offsets are immediates of the reads
  auto read_batch = [](u32x4 (&d)[2][2], unsigned addr, auto tc) __attribute__((always_inline)) {
    constexpr int T = decltype(tc)::value;
    l3_read4<T * 4096, T * 4096 + 512, T * 4096 + 256, T * 4096 + 768>(d, addr);
  };
  // byte address inside a chunk image of (k-step t, block q, part): ((t 4 + g) 2 + part) 32 + 16 q + j units
  const unsigned a_lane = (unsigned)((g * 64 + j) * 16);

  // the two stores of the chunk before: issued behind the next barrier (out of range: dropped)
  u32x4 pend[2];
  unsigned pend_off[2] = {0xFFFFFFF0u, 0xFFFFFFF0u};
  int pend_b = 0;                                                // uniform: they belong to B's output
  pend[0] = pend[1] = (u32x4){0u, 0u, 0u, 0u};
  auto flush = [&]() __attribute__((always_inline)) {
    if (pend_b) {
      __builtin_amdgcn_raw_buffer_store_b128(pend[0], yrs_b, pend_off[0], 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(pend[1], yrs_b, pend_off[1], 0, 0);
    } else {
      __builtin_amdgcn_raw_buffer_store_b128(pend[0], yrs_a, pend_off[0], 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(pend[1], yrs_a, pend_off[1], 0, 0);
    }
  };

  int bufc = 0;                                                  // image of the current chunk; the chunks after it follow in the ring, the one
                                                                 // requested now goes where the chunk before was
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // (the first images: from here on the counted wait below is exact)

  // all chunks of one problem on its resident operand; `nx`: the problem whose chunk 0 follows the last chunk
  auto run = [&](const f16x8 (&xh)[KS], const f16x8 (&xm)[KS], const PxScale& sc, const XresProblem& pr, const XresProblem& nx,
                 const float* bias_lds, const float* winv_lds, int is_b, int m) __attribute__((always_inline)) {
    const int N = pr.N, NC = N / PX_CHUNK;
    const unsigned blk_rows = (unsigned)a.blk_rows, blk_cols = (unsigned)pr.blk_cols;
    const unsigned bb = (unsigned)m / blk_rows;
    const unsigned rowpart = bb * blk_rows * (unsigned)N + ((unsigned)m - bb * blk_rows) * blk_cols;
    const unsigned mask = __builtin_amdgcn_readfirstlane(sc.mask);
#pragma unroll 1
    for (int c = 0; c < NC; ++c) {
      // my pieces of this chunk's image have landed.  Vector memory operations complete in order, and behind those pieces a wave has
      // issued, per chunk since: UPT pieces (of PX_IMAGES - 2 chunks) and, after them, the two stores (of PX_IMAGES - 1 chunks) -- these
      // may still be in flight: the wait does not reach back to a store younger than PX_IMAGES - 1 chunks.  (With the stores in front
      // of the pieces and two images, every barrier waited for the acknowledgement of the stores of the chunk before: 125 us.)
      asm volatile("s_waitcnt vmcnt(%0)" : : "n"((PX_IMAGES - 2) * UPT + (PX_IMAGES - 1) * 2) : "memory");
      __syncthreads();                                           // this chunk's image is complete; the image of the chunk before is free
      const int bufp = bufc == 0 ? PX_IMAGES - 1 : bufc - 1;
      const unsigned a1 = a_lane + (unsigned)(bufc * CHU * 16);
      const unsigned wdma = lds_base + (unsigned)((bufp * CHU + 64 * wave) * 16);   // this wave's first piece of the freed image
      bufc = bufc == PX_IMAGES - 1 ? 0 : bufc + 1;
      read_batch(afr[0], a1, std::integral_constant<int, 0>{});
      read_batch(afr[1], a1, std::integral_constant<int, 1>{});
      const bool wrap = c + PX_IMAGES - 1 >= NC;                 // uniform: the chunk to request is the next problem's (its N: host-checked)
      const XresProblem& np = wrap ? nx : pr;
      const int ncx = wrap ? c + PX_IMAGES - 1 - NC : c + PX_IMAGES - 1;
      const unsigned nvoff = w_voff(np);

      f32x4 acc[2][1];                                           // [block][the wave's one column tile]
      acc[0][0] = acc[1][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // one batch slot = one k-step: this slot's piece of the weight stream, wait for batch T's fragments, request batch T + 2, the
      // schedule's rescaling, six MFMAs
      l3_static_for<0, KS>([&](auto tc) __attribute__((always_inline)) {
        constexpr int T = decltype(tc)::value;
        if constexpr (T == UPT) flush();                         // the stores of the chunk before: behind this chunk's pieces
        if constexpr (T < UPT) l3_glds16(w_base(np, ncx, T), nvoff, wdma + (unsigned)(PX_THREADS * T * 16));
        __builtin_amdgcn_sched_barrier(0);
        l3_wait_lgkm<(T + 1 < KS ? 4 : 0)>(afr[T % 3]);          // (no LDS operation of mine behind the next batch's reads)
        if constexpr (T + 2 < KS) read_batch(afr[(T + 2) % 3], a1, std::integral_constant<int, T + 2>{});
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (T > 0) {                                   // (k-step 0 sets the scale: the accumulators are still zero)
          if ((mask >> T) & 1u) {                                // uniform, rare
            unsigned w = sc.sched[T >> 2];
            asm volatile("" : "+v"(w));                          // (formed here: hoisted, the seven ratios cost 28 registers)
            const float ratio = __builtin_bit_cast(float, ((w >> (8 * (T & 3))) & 255u) << 23);
            acc[0][0] *= ratio;
            acc[1][0] *= ratio;
          }
        }
        const f16x8 bh[1] = {xh[T]}, bm[1] = {xm[T]};
        l3_mfma3_pair<1>(afr[T % 3], bh, bm, acc[0], acc[1]);
        __builtin_amdgcn_sched_barrier(0);
      });

      // D[i = feature][j = row]: a lane holds four consecutive features of its row in each of the two blocks
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int f = PX_CHUNK * c + 16 * q + 4 * g;
        const f32x4 wi = *reinterpret_cast<const f32x4*>(winv_lds + f);
        const f32x4 bi = *reinterpret_cast<const f32x4*>(bias_lds + f);
        const f32x4 v = (acc[q][0] * sc.sx_inv) * wi + bi;          // two exact unscalings, then the bias
        const unsigned cb = (unsigned)f / blk_cols;
        const unsigned off = (rowpart + cb * blk_rows * blk_cols + ((unsigned)f - cb * blk_cols)) * 4u;
        pend[q] = __builtin_bit_cast(u32x4, v);
        pend_off[q] = m < M ? off : 0xFFFFFFF0u;                 // rows past the end store nothing
      }
      pend_b = is_b;
    }
  };

#pragma unroll 1
  for (int grp = blockIdx.x; grp < ngroups; grp += a.nwg) {
    // ---- the wave's tile of x, and of x + add: read once, running scale per k-step, two fp16 parts of both operands in registers
    const int m = grp * PX_ROWS + wave * 16 + j;
    const int mc = min(m, M - 1);                                // rows past the end repeat the last row (never stored)
    const unsigned vo = ((unsigned)mc * (unsigned)K + (unsigned)(8 * g)) * 4u;                                  // < 2^31 (host-checked)
    const unsigned avo = (((unsigned)mc % (unsigned)a.add_rows) * (unsigned)K + (unsigned)(8 * g)) * 4u;
    f16x8 xh_a[KS], xm_a[KS], xh_b[KS], xm_b[KS];
    PxScale sa, sb;
    sa.eset = sb.eset = -1000;
    sa.sx = sa.sx_inv = sb.sx = sb.sx_inv = 1.0f;
    sa.sched[0] = sa.sched[1] = sb.sched[0] = sb.sched[1] = 0u;
    sa.mask = sb.mask = 0u;
    {
      constexpr int RING = KS < 4 ? KS : 4;                      // k-steps of x and of add in flight
      f32x4 rx[RING][2], ra[RING][2];
      auto load_ks = [&](int u, int ks) __attribute__((always_inline)) {
        rx[u][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, vo, ks * 128, 0));
        rx[u][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, vo + 16u, ks * 128, 0));
        ra[u][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, avo, ks * 128, 0));
        ra[u][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ars, avo + 16u, ks * 128, 0));
      };
#pragma unroll
      for (int u = 0; u < RING; ++u) load_ks(u, u);
      __builtin_amdgcn_sched_barrier(0);
      l3_static_for<0, KS>([&](auto tc) __attribute__((always_inline)) {
        constexpr int T = decltype(tc)::value;
        constexpr int u = T % RING;
        px_scale_step<T>(rx[u][0], rx[u][1], sa);
        l3_split8(rx[u][0], rx[u][1], sa.sx, xh_a[T], xm_a[T]);
        const f32x4 s0 = rx[u][0] + ra[u][0], s1 = rx[u][1] + ra[u][1];   // B's operand: one fp32 add per element
        px_scale_step<T>(s0, s1, sb);
        l3_split8(s0, s1, sb.sx, xh_b[T], xm_b[T]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (T + RING < KS) load_ks(u, T + RING);
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    run(xh_a, xm_a, sa, a.p[0], a.p[1], bias_a, winv_a, 0, m);
    run(xh_b, xm_b, sb, a.p[1], a.p[0], bias_b, winv_b, 1, m);
  }
  flush();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // (the last chunks requested the first chunks again: nothing may land after the exit)
}

int linear_pair_xres_f32(const float* x, const float* add, long long add_rows, const void* wp_a, const float* winv_a, const float* bias_a,
                         int N_a, int blk_cols_a, float* y_a, const void* wp_b, const float* winv_b, const float* bias_b, int N_b,
                         int blk_cols_b, float* y_b, long long M, int K, long long blk_rows, void* stream) {
  if (config().linear_ablate == LA_NO_PAIR_XRES) return 0;
  const int n_cu = cu_count();
  if (!pair_xres_covered(M, N_a, N_b, K, add_rows, blk_rows, blk_cols_a, blk_cols_b, n_cu) ||
      !aligned16(x, add, static_cast<const float*>(wp_a), winv_a, bias_a, y_a, static_cast<const float*>(wp_b), winv_b, bias_b, y_b))
    return 0;
  XresArgs a;
  a.X = x; a.add = add; a.M = (int)M; a.add_rows = (int)add_rows; a.blk_rows = (int)blk_rows; a.nwg = (int)pair_xres_grid(M, n_cu);
  a.p[0] = XresProblem{static_cast<const u32x4*>(wp_a), winv_a, bias_a, y_a, N_a, blk_cols_a};
  a.p[1] = XresProblem{static_cast<const u32x4*>(wp_b), winv_b, bias_b, y_b, N_b, blk_cols_b};
  const size_t lds = pair_xres_lds(N_a, N_b, K);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&linear_pair_xres<8>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((linear_pair_xres<8>), dim3((unsigned)a.nwg), dim3(PX_THREADS), lds, static_cast<hipStream_t>(stream), a);
  const int rc = check_launch("linear_pair_xres_f32");
  return rc == UNIVS_OK ? 1 : rc;
}

}  // namespace univs
