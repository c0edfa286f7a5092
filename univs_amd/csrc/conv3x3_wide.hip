// The 3 x 3 convolution of the FPN output (256 -> 256 channels at 1/4 resolution: gemm_f16x3_stream.hip has the GEMM form, M = T H W
// pixels, a k-step = 32 input channels of one tap, k = tap * Cin + ci) with ALL 256 output features of a k-step on one read of x.
//
// WHY: the streamed kernel computes 256 rows x 128 features per workgroup pass, so Cout = 256 is two passes, and each pass walks all nine
// taps: every element of x is fetched from L2 eighteen times, and its row maximum, running scale and two-part split are made eighteen
// times -- and in this family vector work between a wave's matrix instructions adds to its time.  Here a wave's 32 pixels serve 16
// feature blocks: x is loaded, scaled and split once per (tap, 32 channels), the weight image streams through LDS once per row range,
// and there is no second pass.
// ORGANISATION: 8 waves, two per SIMD, 32 pixels per wave as in the streamed kernel; per lane
//   * 128 accumulator registers (16 feature blocks x 2 column tiles);
//   * a register ring of TWO stages of x (16 registers each), refilled two k-steps ahead -- a k-step is twice as long as at 128
//     features, so the lead in time is that of the streamed kernel's four;
//   * A fragments in eight batches of two feature blocks, two buffers (32 registers), read one batch ahead (f16x3_kstep.h);
//   * W: a k-step's 256-feature slab is 32 contiguous KB of the pre-split image (units (kc 2 + part) N + r).  It goes global -> LDS by DMA
//     (l3_glds16 of f16x3_wstream.h) into four images = two PAIRS of k-steps: one barrier per pair, behind it the pair after
//     this one is requested into the images the pair before has left.  (One barrier per k-step with the k-step three ahead requested
//     measured 25-40 us more on the NCHW operand: two waves of a SIMD that meet at every k-step do their vector work, and then their
//     matrix work, at the same time.)  The ring runs on across tiles and rounds (the same W for every row: k-step indices wrap).
// ARITHMETIC: an output's value depends on its row of W, its row of x in k order and that row's running-scale sequence only
// (linear_pair_xres.hip); all three are the streamed kernel's -- the same l3_* helpers, the lowering vote over the same 32 rows, the
// three products in f16x3.h's order -- so y has the bits of gemm_f16x3_stream<8, 4, XMODE> (tests/test_conv3x3_wide_gpu.py).
// Covered, row ranges: conv3x3_wide_plan.h.  profiles/conv3x3_wide_resources_v1.txt has the build's register, LDS and scratch figures.
// MEASURED (profiles/conv3x3_wide_clip_breakdown_{parent,this}.txt, 294 400 pixels, NCHW): see DESIGN.md, "The FPN 3 x 3 convolution
// with all 256 features per read of x"; profiles/conv3x3_wide_ablation_v1.txt has the kernel without its split / matrix instructions.
#include "common.h"
#include "config.h"
#include "conv3x3_wide_plan.h"
#include "f16x3_kstep.h"
#include "f16x3_wstream.h"
#include "launchers.h"

namespace univs {

struct CwArgs {
  const float* X;                // XMODE 1: [T, Cin, H, W]; XMODE 2: [T, H, W, Cin]
  const u32x4* Wp;               // the pre-split image of presplit_f16x3 (conv k order): [(9 Cin / 8) x 2 parts][256] 16-byte units
  const float* winv;             // [256] inverse row scales of the image
  float* Y;                      // [T, 256, H, W]
  int M, Cin, H, Wd, HW, rounds; // rounds: of every workgroup but the last (plan_conv3x3_wide)
};

template <int XMODE>
__global__ __launch_bounds__(CW_THREADS) void conv3x3_wide(const CwArgs a) {
  static_assert(XMODE == 1 || XMODE == 2, "operand layouts");
  extern __shared__ __attribute__((aligned(16))) u32x4 Lds[];
  constexpr int RB = CW_COUT / 16;                               // feature blocks of a wave
  constexpr int IMG = 4 * 2 * CW_COUT;                           // 16-byte units of a k-step image: [k-group][part][feature]
  constexpr int NWV = CW_THREADS / 64;
  constexpr int UPT = IMG / CW_THREADS;                          // DMA pieces per wave and k-step
  constexpr int XL = XMODE == 1 ? 16 : 4;                        // vector loads of one stage of x
  constexpr int NB = RB / 2;                                     // fragment batches of two feature blocks
  static_assert(IMG % CW_THREADS == 0 && CW_IMAGES == 4 && 2 * XL < 64, "stream geometry");
  const int M = a.M;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int kspt = a.Cin >> 5, KS = 9 * kspt;                    // k-steps per tap (a multiple of 4), per tile
  const int WT = (M + CW_TILE_M - 1) / CW_TILE_M;
  const int rd0 = (int)blockIdx.x * a.rounds;                    // my rounds of the sequence
  const int rounds = min(a.rounds, (WT + NWV - 1) / NWV - rd0);  // every wave runs all rounds (barriers); idle tiles store nothing
  if (rounds <= 0) return;
  float* winv_lds = reinterpret_cast<float*>(Lds + CW_IMAGES * IMG);
  for (int r = tid; r < CW_COUT; r += CW_THREADS) winv_lds[r] = a.winv[r];

  // ---- weight stream: piece v of k-step s = units s IMG + CW_THREADS v + tid of the split image -> the same place of an LDS image
  const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)Lds);
  const unsigned w_voff = (unsigned)tid * 16u;
  auto w_request = [&](int s, int img) __attribute__((always_inline)) {
    const u32x4* base = a.Wp + (size_t)s * IMG;
    const unsigned dst = lds_base + (unsigned)((img * IMG + 64 * wave) * 16);
#pragma unroll
    for (int v = 0; v < UPT; ++v) l3_glds16(base + CW_THREADS * v, w_voff, dst + (unsigned)(CW_THREADS * v * 16));
  };
#pragma unroll
  for (int s = 0; s < 2; ++s) w_request(s, s);                   // the first pair of k-steps

  // ---- x: the streamed kernel's addressing (gemm_f16x3_stream.hip, XMODE 1 / 2), all nine taps
  const long long xbytes = (long long)(M / a.HW) * a.Cin * a.HW * 4;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.X), 0, (int)xbytes, 0x00020000);
  const long long ybytes = (long long)(M / a.HW) * CW_COUT * a.HW * 4;
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(a.Y, 0, (int)ybytes, 0x00020000);
  struct TileRows {                                              // per column tile: byte offset of (frame, channel 8 g, pixel) + pixel coords
    unsigned vo[2];
    int py[2], px[2];
  };
  auto tile_rows = [&](int tt, TileRows& t) __attribute__((always_inline)) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int m = min(tt * CW_TILE_M + 16 * c + j, M - 1);     // rows past the end repeat the last row (not stored)
      const int f = m / a.HW, rem = m - f * a.HW;
      t.py[c] = rem / a.Wd;
      t.px[c] = rem - t.py[c] * a.Wd;
      t.vo[c] = XMODE == 2 ? ((unsigned)m * (unsigned)a.Cin + (unsigned)(8 * g)) * 4u
                           : (unsigned)((f * a.Cin + 8 * g) * a.HW + rem) * 4u;
    }
  };
  // 8 input channels 32 kc + 8 g .. of tap `tap` at my (shifted) pixels; taps outside the image read 0 (offset out of range)
  auto load_x = [&](f32x4 (&buf)[2][2], const TileRows& t, int tap, int kc) __attribute__((always_inline)) {
    const int cb = kc * 32;                                      // uniform
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const bool inb = (unsigned)(t.py[c] + dy) < (unsigned)a.H && (unsigned)(t.px[c] + dx) < (unsigned)a.Wd;
      if (XMODE == 2) {
        const unsigned vo = inb ? t.vo[c] + (unsigned)((dy * a.Wd + dx) * a.Cin * 4) : 0xFFFFFFE0u;
        buf[c][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, vo, cb * 4, 0));
        buf[c][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, vo + 16u, cb * 4, 0));
      } else {
        const unsigned vo = inb ? t.vo[c] + (unsigned)((dy * a.Wd + dx) * 4) : 0xFFFFFFF0u;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          buf[c][e >> 2][e & 3] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xrs, vo, (cb + e) * a.HW * 4, 0));
      }
    }
  };

  // ---- A fragments: batch b = feature blocks 2 b, 2 b + 1 of the image at lane address `base`; block (256 B) and part (4 KB) offsets
  // are immediates of the reads
  typedef u32x4 Batch[2][2];                                     // [block of the batch][part h, m]
  auto read_batch = [](Batch& d, unsigned base, auto bc) __attribute__((always_inline)) {
    constexpr int b = decltype(bc)::value;
    l3_read4<b * 512, b * 512 + CW_COUT * 16, b * 512 + 256, b * 512 + 256 + CW_COUT * 16>(d, base);
  };
  const unsigned a_lane = (unsigned)((g * 2 * CW_COUT + j) * 16);

  f32x4 acc[RB][2];
  int eset[2];
  float sx[2], sx_inv[2];
  Batch afr[2];
  f32x4 raw[2][2][2];                                            // [stage][column tile][8 k-values]

  // the loader runs two k-steps ahead of the products, across tiles: t_ld is the tile it reads, (ld_tap, ld_kc) its next k-step
  TileRows t_ld, t_nx;
  tile_rows(rd0 * NWV + wave, t_ld);
  tile_rows((rd0 + min(1, rounds - 1)) * NWV + wave, t_nx);
  load_x(raw[0], t_ld, 0, 0);
  load_x(raw[1], t_ld, 0, 1);
  int ld_tap = 0, ld_kc = 2;                                     // (kspt >= 4)
  int img = 0;                                                   // image of the current k-step; the next k-step's follows it in the ring
  int sreq = 2;                                                  // the k-step requested next (mod KS; KS is even)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // (the first images: from here on the counted wait below is exact)

#pragma unroll 1
  for (int rd = 0; rd < rounds; ++rd) {
    const int tt = (rd0 + rd) * NWV + wave;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb][0] = acc[rb][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
    l3_row_scale_reset(eset, sx, sx_inv);
#pragma unroll 1
    for (int q = 0; q < KS; q += 2) {
      l3_static_for<0, 2>([&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value;
        if constexpr (u == 0) {
          // one barrier per PAIR of k-steps.  My pieces of this pair's images have landed: vector memory operations complete in order,
          // and behind those pieces a wave has issued the two x stages of the pair before (XL loads each) -- those may still be in
          // flight; the stores of an epilogue in between only make the wait reach further back
          asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * XL) : "memory");
          __syncthreads();                                       // this pair's images are complete; the images of the pair before are free
          w_request(sreq, (img + 2) & (CW_IMAGES - 1));
          w_request(sreq + 1, (img + 3) & (CW_IMAGES - 1));
          sreq = sreq + 2 == KS ? 0 : sreq + 2;
        }
        const unsigned a_buf = a_lane + (unsigned)(img * IMG * 16);
        img = (img + 1) & (CW_IMAGES - 1);
        read_batch(afr[0], a_buf, std::integral_constant<int, 0>{});
        // ---- the running row scale (f16x3_kstep.h)
        int enew[2];
        if (__builtin_amdgcn_ballot_w64(l3_row_scale_need(raw[u], eset, enew)) != 0) l3_row_scale_lower<RB>(enew, acc, eset, sx, sx_inv);
        float s0 = sx[0], s1 = sx[1];
        asm volatile("" : "+v"(s0), "+v"(s1) : : "memory");
        f16x8 bh[2], bm[2];
        l3_split8(raw[u][0][0], raw[u][0][1], s0, bh[0], bm[0]);
        l3_split8(raw[u][1][0], raw[u][1][1], s1, bh[1], bm[1]);
        __builtin_amdgcn_sched_barrier(0);
        load_x(raw[u], t_ld, ld_tap, ld_kc);                     // the stage just split: its k-step two ahead
        if (++ld_kc == kspt) {                                   // uniform
          ld_kc = 0;
          if (++ld_tap == 9) {                                   // the next tile (the last round reads its own tile again: never used)
            ld_tap = 0;
            t_ld = t_nx;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        l3_static_for<0, NB>([&](auto bc) __attribute__((always_inline)) {
          constexpr int b = decltype(bc)::value;
          l3_wait_batch(afr[b & 1]);
          if constexpr (b + 1 < NB) read_batch(afr[(b + 1) & 1], a_buf, std::integral_constant<int, b + 1>{});
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int qb = 0; qb < 2; ++qb)                         // one feature block after the other, as l3_mfma_batch
            l3_mfma3_block<2>(__builtin_bit_cast(f16x8, afr[b & 1][qb][0]), __builtin_bit_cast(f16x8, afr[b & 1][qb][1]), bh, bm, acc[2 * b + qb]);
          __builtin_amdgcn_sched_barrier(0);
        });
      });
    }
    // ---- epilogue: D[i = feature][j = row]: a lane holds four consecutive features of its two pixels; NCHW: four channel planes
    const bool tile_ok = tt < WT;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int m = tt * CW_TILE_M + 16 * c + j;
      const bool row_ok = tile_ok && m < M;
      const int fr = min(m, M - 1) / a.HW, rem = min(m, M - 1) - fr * a.HW;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const int f = rb * 16 + 4 * g;
        const f32x4 wi = *reinterpret_cast<const f32x4*>(winv_lds + f);
        // two exact unscalings; `+ 0`: the streamed kernel's (absent) bias, which turns a -0 into +0
        const f32x4 v = (acc[rb][c] * sx_inv[c]) * wi + (f32x4){0.f, 0.f, 0.f, 0.f};
        // out-of-range lanes move their offset out of the buffer
        const unsigned off0 = row_ok ? (unsigned)((fr * CW_COUT + f) * a.HW + rem) * 4u : 0xFFFFFFF0u - 3u * (unsigned)a.HW * 4u;
        float vx = v.x, vy = v.y, vz = v.z, vw = v.w;
        asm volatile("" : "+v"(vx), "+v"(vy), "+v"(vz), "+v"(vw));   // (gemm_f16x3_stream.hip: hipcc 7.2 stored the first element four times without this)
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vx), yrs, off0, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vy), yrs, off0 + (unsigned)a.HW * 4u, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vz), yrs, off0 + 2u * (unsigned)a.HW * 4u, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vw), yrs, off0 + 3u * (unsigned)a.HW * 4u, 0, 0);
      }
    }
    tile_rows((rd0 + min(rd + 2, rounds - 1)) * NWV + wave, t_nx);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");               // (the last k-steps requested images again: nothing may land after the exit)
}

int conv3x3_wide_f32(int xmode, const float* x, const void* wp, const float* winv, float* y, int T, int Cin, int Cout, int H, int W,
                     hipStream_t st) {
  if (config().linear_ablate == LA_NO_CONV_WIDE || T <= 0 || H <= 0 || W <= 0) return 0;
  const long long M = (long long)T * H * W;
  if (!conv3x3_wide_covered(M, Cin, Cout) || !aligned16(x, wp, y, winv)) return 0;
  const WidePlan p = plan_conv3x3_wide(M, cu_count());
  CwArgs a;
  a.X = x; a.Wp = reinterpret_cast<const u32x4*>(wp); a.winv = winv; a.Y = y;
  a.M = (int)M; a.Cin = Cin; a.H = H; a.Wd = W; a.HW = H * W; a.rounds = p.rounds;
  const size_t lds = conv3x3_wide_lds();
  if (xmode == 2) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_wide<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((conv3x3_wide<2>), dim3(p.nwg), dim3(CW_THREADS), lds, st, a);
  } else {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_wide<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((conv3x3_wide<1>), dim3(p.nwg), dim3(CW_THREADS), lds, st, a);
  }
  const int rc = check_launch("conv3x3_wide_f32");
  return rc == UNIVS_OK ? 1 : rc;
}

}  // namespace univs
