// Swin window attention that computes q, k, v itself: image-mode attention on 7 x 7 windows, head_dim 32, three-product arithmetic
// (UNIVS_MMA_F16X3), C = K in {96, 192} (Swin-T/S stages 1 and 2), from the NORMALISED TOKENS x [B, H*W, C] and the cached split image of
// qkv.weight.  The [B, H*W, 3C] tensor of the qkv Linear -- written by one launch to be read once by the next -- does not exist.
//
// Two texts meet here, both unchanged in their arithmetic, so the output has the bits of the two launches it replaces:
//   * the projection is one pass of the W-resident Linear (linear_f16x3.hip) built from the family's k-step core (f16x3_kstep.h: k order,
//     running row scale, split, product order), with that kernel's epilogue expression (acc * sx_inv) * winv + bias.  A pass kernel's result
//     for (row, feature) depends only on that row of x, that row of W and the row's running scale, so WHICH rows share a tile is free;
//   * everything after q, k, v is window_attn_img_f16<4, false, 3> (window_attn_f16.hip), duplicated below from "range tests" on.
//
// Organisation (as window_attn_img_f16): a workgroup = 8 waves = ONE head, persistent over windows; a wave = one window at a time;
// pad / roll / partition / reverse / crop by index arithmetic (`token()`, WinImage).
//   * Once per workgroup, beside the bias table, the head's 96 rows of W (q, k, v x 32 channels) go into LDS in KStep<6> order
//     ([k-step][4 k-groups][2 parts][96] 16-byte units): a copy from the split image (unit (kc 2 + part) N + r, kc = 4 ks + g) with a row
//     map, plus the 96 inverse row scales and qkv biases.  LDS row 32 p + 16 b + 4 g + e (p = q, k, v; b in {0, 1}) is head channel
//     8 g + 4 b + e: the accumulator layout D[i = feature][j = row] then leaves lane (n, g) with channels 8g .. 8g+7 of row n in
//     acc[2p][c], acc[2p+1][c] -- exactly the kf / qf fragment the attention builds from global memory, in the same element order.
//     K and Q need no data movement; V goes through the per-wave `vt` staging (fp16 parts, transposed), written from the accumulators.
//   * Per window two row tiles of 32 (column tiles jb = 2 tile + c), each one pass of the Linear's k-loop over KS = K / 32 k-steps with a
//     ring of three stages of x.  A zero-padded pixel is a row of zeros (a buffer load out of range): 0 * ... + bias = bias, the q/k/v the
//     two-launch path takes from qkv_bias.  Rows >= 49 are set to 0 after the projection, as that path's missing row pointer leaves them.
//   * The heads of a window range read the same rows of x: the workgroup -> (window range, head) map puts them on one XCD (xcd_remap),
//     where the re-reads meet in L2.
// LDS at 8 waves: W image 12 288 KS, bias table 17 408, V staging 8 x 8 704, 768 of bias / winv: 124 672 B (K = 96), 161 536 B (K = 192).
#include "common.h"
#include "config.h"
#include "f16x3_kstep.h"
#include "window_attn.h"
#include "launchers.h"

#include <algorithm>

namespace univs {

// (window_attn_f16.hip: wh_wave_scale, wh_out_of_range -- the same text under names of this file)
__device__ __forceinline__ void wq_wave_scale(float mx, float& s, float& inv) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  int e = (int)((__builtin_bit_cast(unsigned, mx) >> 23) & 255u) - 127;   // 2^e <= max < 2^(e+1)
  e = max(-40, min(e, 128));
  s = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane((127 + 14 - e) << 23));
  inv = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane((127 - 14 + e) << 23));
}
__device__ __forceinline__ bool wq_out_of_range(float mx, float lo) {
  return __builtin_amdgcn_ballot_w64(!(mx < 32768.0f)) != 0 || __builtin_amdgcn_ballot_w64(mx >= lo) == 0;
}

typedef f32x4 __attribute__((may_alias)) wq_f32x4_a;          // (the V staging area holds fp32 vectors for a while)
constexpr int WQ_WAVES = 8, WQ_HD = 32, WQ_NB = 4, WQ_NP = 64, WQ_BS = WQ_NP + 4, WQ_VS = WQ_NP + 4, WQ_RB = 6, WQ_RP = 16 * WQ_RB;
constexpr size_t wq_lds_bytes(int KS) {
  return (size_t)KS * 8 * WQ_RP * 16 + (size_t)WQ_NP * WQ_BS * 4 + (size_t)WQ_WAVES * 2 * WQ_HD * WQ_VS * 2 + 2 * WQ_RP * 4;
}

template <int KS>   // k-steps of 32: C = 32 KS
__global__ __launch_bounds__(64 * WQ_WAVES) void window_attn_qkv_f16x3(const float* __restrict__ x,          // [B, H*W, C]
                                                                        const u32x4* __restrict__ wp,         // split image of qkv.weight
                                                                        const float* __restrict__ winv,       // [3C]
                                                                        const float* __restrict__ qkv_bias,   // [3C] or null
                                                                        const float* __restrict__ bias,       // [nH, 49, 49]
                                                                        const float* __restrict__ shift_mask, int B_, int nW, int nH,
                                                                        int gx, int xbytes, float scale, float* __restrict__ out,
                                                                        WinImage wi, int magic) {
  constexpr int HD = WQ_HD, NB = WQ_NB, NP = WQ_NP, BS = WQ_BS, VS = WQ_VS, RB = WQ_RB, Rp = WQ_RP, C = 32 * KS, RING = 3;
  constexpr int NTHREADS = 64 * WQ_WAVES;
  constexpr float LOG2E = 1.4426950408889634f;
  const int Ntok = wi.ws * wi.ws;
  extern __shared__ __attribute__((aligned(16))) u32x4 lds_wq[];
  u32x4* Wsp = lds_wq;                                          // [KS][4 k-groups][2 parts][Rp]: at LDS address 0 (the batch reader's base)
  float* bias_lds = reinterpret_cast<float*>(Wsp + KS * 8 * Rp);   // [NP][BS]: log2e * bias of head h, -inf for keys >= Ntok
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  _Float16* vt = reinterpret_cast<_Float16*>(bias_lds + NP * BS) + wave * (2 * HD * VS);   // [2 parts][HD][VS]
  float* qb_lds = reinterpret_cast<float*>(reinterpret_cast<_Float16*>(bias_lds + NP * BS) + WQ_WAVES * (2 * HD * VS));   // [Rp] qkv bias
  float* wv_lds = qb_lds + Rp;                                  // [Rp] inverse row scales of W
  // workgroup -> (window range bx, head h): heads minor, every XCD a contiguous chunk of the sequence
  const unsigned lw = xcd_remap(blockIdx.x, gridDim.x);
  const int bx = (int)(lw / (unsigned)nH), h = (int)lw - bx * nH;
  const int g = lane >> 4, n = lane & 15;

  // ---- once per workgroup: bias table, the head's rows of W in fragment order, their scales and biases
  for (int idx = threadIdx.x; idx < NP * NP; idx += NTHREADS) {
    const int i = idx / NP, j = idx - i * NP;
    float v = j < Ntok ? 0.f : -INFINITY;
    if (i < Ntok && j < Ntok) v = bias[((long long)h * Ntok + i) * Ntok + j] * LOG2E;
    bias_lds[i * BS + j] = v;
  }
  // LDS row R = 32 p + 16 b + 4 gg + e  <-  row p C + 32 h + 8 gg + 4 b + e of qkv.weight
  auto w_row = [&](int R) __attribute__((always_inline)) -> int {
    const int p = R >> 5, b = (R >> 4) & 1, gg = (R >> 2) & 3, e = R & 3;
    return p * C + h * HD + 8 * gg + 4 * b + e;
  };
  for (int idx = threadIdx.x; idx < KS * 8 * Rp; idx += NTHREADS) {
    const int run = idx / Rp, R = idx - run * Rp;               // run = kc 2 + part
    Wsp[idx] = wp[(size_t)run * (3 * C) + w_row(R)];
  }
  for (int R = threadIdx.x; R < Rp; R += NTHREADS) {
    const int r = w_row(R);
    qb_lds[R] = qkv_bias ? qkv_bias[r] : 0.f;
    wv_lds[R] = winv[r];
  }
  __syncthreads();   // the only workgroup barrier: every wave reaches it, with or without a window

  const int nWy = wi.Hp / wi.ws;
  const float qscale = scale * LOG2E;    // scores in the exp2 domain
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, xbytes, 0x00020000);
  using KS_ = KStep<RB>;
  constexpr int KNB = KS_::NB;
  const unsigned a_lane = KS_::lane(g, n);
  auto read_batch = l3_batch_reader<RB>();

#pragma unroll 1
  for (int b = bx * WQ_WAVES + wave; b < B_; b += gx * WQ_WAVES) {   // scalar
    const int w = b % nW, img = b / nW;
    const int wy = w / wi.nWx, wx = w - wy * wi.nWx;
    const int y0 = wy * wi.ws + wi.shift, x0 = wx * wi.ws + wi.shift;
    const bool masked = shift_mask && (wy == nWy - 1 || wx == wi.nWx - 1);   // scalar
    // token of row j: >= 0 its index, -1 a zero-padded pixel (q/k/v = the qkv bias), -2 beyond Ntok
    auto token = [&](int j) __attribute__((always_inline)) -> int {
      const int py = (j * magic) >> 16, px = j - py * wi.ws;
      int y = y0 + py, xx = x0 + px;
      y -= (y >= wi.Hp) ? wi.Hp : 0;
      xx -= (xx >= wi.Wp) ? wi.Wp : 0;
      const int t = (y < wi.H && xx < wi.W) ? (img * wi.H + y) * wi.W + xx : -1;
      return j < Ntok ? t : -2;
    };
    int tok[NB];                     // of my rows j = 16 jb + n
    int nt = n;
    asm volatile("" : "+v"(nt));     // (see below: lane coordinates made opaque per phase)
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) tok[jb] = token(jb * 16 + nt);

    // ---- q, k, v of the window's 64 rows: two passes of the Linear's k-loop (linear_f16x3.hip: `group`), 2 KS steps in all.
    // x as the Linear loads it: lane (j, g) takes two 16-byte loads of row j at k-group g per k-step; a row without a token reads
    // out of the buffer's range, i.e. zeros.
    unsigned vo[NB];
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) vo[jb] = tok[jb] >= 0 ? ((unsigned)tok[jb] * (unsigned)C + (unsigned)(8 * g)) * 4u : 0x80000000u;
    f32x4 raw[RING][2][2];                                       // [stage][column tile][16-byte half]
    auto load_x = [&](f32x4 (&buf)[2][2], int tile, int ks) __attribute__((always_inline)) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        buf[c][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, vo[2 * tile + c], ks * 128, 0));
        buf[c][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, vo[2 * tile + c] + 16u, ks * 128, 0));
      }
    };
#pragma unroll
    for (int u = 0; u < RING; ++u) {
      load_x(raw[u], 0, u);                                      // RING <= KS
      __builtin_amdgcn_sched_barrier(0);
    }
    float qraw[NB][8], kraw[NB][8], vraw[NB][8];                 // fp32 rows of q, k, v: channels 8g .. 8g+7 of row 16 jb + n
    // Registers: the second tile's accumulators, x ring and W fragments leave no room for all 48 results of the first, so its q and k
    // (32 registers) wait in this wave's V staging area, which is idle until the projection is done: 8 conflict-free 16-byte slots per lane
    wq_f32x4_a* stash = reinterpret_cast<wq_f32x4_a*>(vt);       // 8 x 1 024 B of the wave's 8 704
    l3_static_for<0, 2>([&](auto tc) __attribute__((always_inline)) {
      constexpr int tile = decltype(tc)::value;
      f32x4 acc[RB][2];
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) acc[rb][0] = acc[rb][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
      int eset[2];                                               // the running scale of my two rows (f16x3_kstep.h)
      float sx[2], sx_inv[2];
      l3_row_scale_reset(eset, sx, sx_inv);
      typename KS_::Batch afr[2];                                // [buffer]: the batch in use and the one being read
      read_batch(afr[0], a_lane, std::integral_constant<int, 0>{});
      l3_static_for<0, KS>([&](auto kc) __attribute__((always_inline)) {
        constexpr int ks = decltype(kc)::value;
        constexpr int step = tile * KS + ks, u = step % RING;
        int enew[2];
        if (__builtin_amdgcn_ballot_w64(l3_row_scale_need(raw[u], eset, enew)) != 0) l3_row_scale_lower(enew, acc, eset, sx, sx_inv);   // rare
        float s0 = sx[0], s1 = sx[1];
        asm volatile("" : "+v"(s0), "+v"(s1) : : "memory");    // pins the consumption of ring stage u here
        f16x8 bh[2], bm[2];
        l3_split8(raw[u][0][0], raw[u][0][1], s0, bh[0], bm[0]);
        l3_split8(raw[u][1][0], raw[u][1][1], s1, bh[1], bm[1]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (step + RING < 2 * KS) load_x(raw[u], (step + RING) / KS, (step + RING) % KS);   // refill the stage just consumed
        __builtin_amdgcn_sched_barrier(0);
        l3_static_for<0, KNB>([&](auto bc) __attribute__((always_inline)) {
          constexpr int bb = decltype(bc)::value;
          l3_wait_batch(afr[bb & 1]);
          if constexpr (bb + 1 < KNB) read_batch(afr[(bb + 1) & 1], a_lane + (unsigned)ks * KS_::kstep, std::integral_constant<int, bb + 1>{});
          else if constexpr (ks + 1 < KS) read_batch(afr[0], a_lane + (unsigned)(ks + 1) * KS_::kstep, std::integral_constant<int, 0>{});
          __builtin_amdgcn_sched_barrier(0);
          l3_mfma_batch<RB, bb>(afr[bb & 1], bh, bm, acc);
          __builtin_amdgcn_sched_barrier(0);
        });
      });
      // the Linear's epilogue expression; feature rb 16 + 4g + r = LDS row -> p = rb / 2, channel 8g + 4 (rb & 1) + r
      // (the address is made opaque here: the 12 scale and bias vectors are the same for every window, and hipcc otherwise keeps all
      // 48 registers of them alive across the window loop)
      const float* qbp = qb_lds + 4 * g;
      asm volatile("" : "+v"(qbp));
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int jb = 2 * tile + c;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          const f32x4 wi4 = *reinterpret_cast<const f32x4*>(qbp + Rp + rb * 16);
          const f32x4 bi4 = *reinterpret_cast<const f32x4*>(qbp + rb * 16);
          f32x4 v = (acc[rb][c] * sx_inv[c]) * wi4 + bi4;          // two exact unscalings, then the bias
          if (jb == NB - 1 && tok[jb] == -2) v = (f32x4){0.f, 0.f, 0.f, 0.f};   // rows >= Ntok (block 3 only: Ntok = 49)
          if (tile == 0 && rb < 4) {
            stash[(c * 4 + rb) * 64 + lane] = v;                  // q, k of the first tile wait in LDS
          } else {
            float* dst = rb < 2 ? qraw[jb] : (rb < 4 ? kraw[jb] : vraw[jb]);
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[4 * (rb & 1) + e] = v[e];
          }
        }
      }
    });
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const f32x4 v = stash[(c * 4 + rb) * 64 + lane];
        float* dst = rb < 2 ? qraw[c] : kraw[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[4 * (rb & 1) + e] = v[e];
      }

    // ======== from here on: window_attn_img_f16<4, false, 3> (window_attn_f16.hip), its operands in registers instead of in memory
    // (lane coordinates made opaque per phase: what hipcc derives from them -- mask indices, V addresses, token rows -- is the same for
    // every window, and hoisted out of the window loop it held ~60 registers through the projection, which has none to spare)
    int na = n, ga = g;
    asm volatile("" : "+v"(na), "+v"(ga));
    // ---- V: range test, split, transposed into LDS as fp16 parts ([part][channel][key]); a lane holds 8 channels of ONE key per block
    float sv_inv = 1.0f;                                           // inverse of the power of two applied to V (rarely != 1)
    {
      float mv = 0.f;
#pragma unroll
      for (int jb = 0; jb < NB; ++jb)
#pragma unroll
        for (int e = 0; e < 8; e += 2) mv = fmaxf(mv, fmaxf(fabsf(vraw[jb][e]), fabsf(vraw[jb][e + 1])));
      if (wq_out_of_range(mv, 0.0625f)) {
        float sv;
        wq_wave_scale(mv, sv, sv_inv);
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
#pragma unroll
          for (int e = 0; e < 8; ++e) vraw[jb][e] *= sv;
      }
    }
#pragma unroll
    for (int jb = 0; jb < NB; ++jb) {
      f16x8 vh, vm;
      l3_split8(vraw[jb], vh, vm);
      _Float16* dst = vt + (8 * ga) * VS + jb * 16 + na;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        dst[e * VS] = vh[e];
        dst[HD * VS + e * VS] = vm[e];
      }
    }

    // ---- K fragments: lane holds K[jb*16 + n][8g .. 8g+7] as 8 halves, two parts
    f16x8 kf[NB], kfm[NB];
    float sk = 1.0f, sk_inv = 1.0f;                              // power of two applied to K (rarely != 1)
    {
      float mk = 0.f;
#pragma unroll
      for (int jb = 0; jb < NB; ++jb)
#pragma unroll
        for (int e = 0; e < 8; e += 2) mk = fmaxf(mk, fmaxf(fabsf(kraw[jb][e]), fabsf(kraw[jb][e + 1])));
      if (wq_out_of_range(mk, 0.0625f)) {
        wq_wave_scale(mk, sk, sk_inv);
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
#pragma unroll
          for (int e = 0; e < 8; ++e) kraw[jb][e] *= sk;
      }
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) l3_split8(kraw[jb], kf[jb], kfm[jb]);
    }
    const float* mask_w = masked ? shift_mask + (long long)w * Ntok * Ntok : nullptr;
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes are visible to its own reads
    __builtin_amdgcn_wave_barrier();

    // the query loop stays rolled (as in the origin); the block's q comes out of the four register rows by a scalar select
#pragma unroll 1
    for (int ib = 0; ib < NB; ++ib) {
      const int i = ib * 16 + na;        // this lane's query (column of S^T)
      const int tok_i = token(i);
      f16x8 qf, qfm;
      float ss = 1.0f, ss_inv = 1.0f;                             // wave-uniform (scalar registers)
      {
        float qq[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float q01 = ib == 0 ? qraw[0][e] : qraw[1][e], q23 = ib == 2 ? qraw[2][e] : qraw[3][e];
          qq[e] = (ib < 2 ? q01 : q23) * qscale;
        }
        // BOTH parts must come from the fp32-ROUNDED product (window_attn_f16.hip has the story)
#pragma unroll
        for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(qq[e]));
        float mq = 0.f;                                          // range test of the scaled queries of this block
#pragma unroll
        for (int e = 0; e < 8; e += 2) mq = fmaxf(mq, fmaxf(fabsf(qq[e]), fabsf(qq[e + 1])));
        float sq = 1.0f, sq_inv = 1.0f;
        if (wq_out_of_range(mq, 0.015625f)) {
          wq_wave_scale(mq, sq, sq_inv);
#pragma unroll
          for (int e = 0; e < 8; ++e) qq[e] *= sq;
        }
        ss = sk * sq;                                           // the scores come out of the matrix cores times ss
        ss_inv = sk_inv * sq_inv;
        l3_split8<true>(qq, qf, qfm);                            // (the parts go straight into the matrix instructions)
      }
      f32x4 s[NB];
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) {
        // bias (and the -inf of the padded keys) is the accumulator's initial value
        const f32x4 acc = *reinterpret_cast<const f32x4*>(bias_lds + i * BS + jb * 16 + 4 * ga);
        f32x4 sc = acc;
        if (ss != 1.0f) sc = acc * ss;                          // scalar: only windows that needed a range scale
        sc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kfm[jb], qf, sc, 0, 0, 0);   // smallest terms first
        sc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[jb], qfm, sc, 0, 0, 0);
        s[jb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[jb], qf, sc, 0, 0, 0);
      }
      if (ss != 1.0f) {                                         // scalar
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) s[jb] *= ss_inv;
      }
      if (mask_w) {   // scalar: last row / column of windows only
        // unconditional loads at clamped indices + a select (see window_attn.hip)
        const float* mrow = mask_w + min(i, Ntok - 1) * Ntok;
#pragma unroll
        for (int jb = 0; jb < NB; ++jb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int j = jb * 16 + 4 * ga + r;
            const float mv = mrow[min(j, Ntok - 1)];
            s[jb][r] += (i < Ntok && j < Ntok) ? mv * LOG2E : 0.f;
          }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int jb = 0; jb < NB; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[jb][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float sum = 0.f;
      f16x4 p[NB], pm[NB];
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) {
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          e[r] = __builtin_amdgcn_exp2f(s[jb][r] - mx);          // exp2(-inf) = 0 for padded keys
          sum += e[r];
        }
        l3_split4<true>(e[0], e[1], e[2], e[3], p[jb], pm[jb]);   // (from v_exp_f32 into the matrix instructions)
      }
      sum += __shfl_xor(sum, 16);
      sum += __shfl_xor(sum, 32);
      const float inv = (1.0f / sum) * sv_inv;     // of query n (the same value in the four lane groups); V's range scale undone

      // out[ib] (16 queries x 32 channels) = P[ib, :] @ V : two 16-channel halves
      f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int jb = 0; jb < NB; ++jb) {
        const f16x4 b0 = *reinterpret_cast<const f16x4*>(vt + na * VS + jb * 16 + 4 * ga);
        const f16x4 b1 = *reinterpret_cast<const f16x4*>(vt + (16 + na) * VS + jb * 16 + 4 * ga);
        const f16x4 b0m = *reinterpret_cast<const f16x4*>(vt + HD * VS + na * VS + jb * 16 + 4 * ga);
        const f16x4 b1m = *reinterpret_cast<const f16x4*>(vt + HD * VS + (16 + na) * VS + jb * 16 + 4 * ga);
        o0 = __builtin_amdgcn_mfma_f32_16x16x16f16(pm[jb], b0, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x16f16(pm[jb], b1, o1, 0, 0, 0);
        o0 = __builtin_amdgcn_mfma_f32_16x16x16f16(p[jb], b0m, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x16f16(p[jb], b1m, o1, 0, 0, 0);
        o0 = __builtin_amdgcn_mfma_f32_16x16x16f16(p[jb], b0, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x16f16(p[jb], b1, o1, 0, 0, 0);
      }
      // C layout: row = 4g + r -> query ib*16 + 4g + r (token and 1/sum: lane 4g + r); col = n -> channel n / 16 + n
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = __shfl(tok_i, 4 * ga + r, 64);
        const float invr = __shfl(inv, 4 * ga + r, 64);
        if (t >= 0) {
          float* op = out + ((long long)t * nH + h) * HD;
          op[na] = o0[r] * invr;
          op[16 + na] = o1[r] * invr;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();   // the next window's V staging overwrites vt
  }
}

template <int KS>
static int launch_wq(const float* x, const void* wp, const float* winv, const float* qkv_bias, const float* bias, const float* shift_mask,
                     int B_, int nW, int nH, long long xbytes, float scale, float* out, const WinImage& wi, int n_cu, hipStream_t st) {
  const size_t lds = wq_lds_bytes(KS);                          // one workgroup per CU
  // workgroups = CUs rounded DOWN to a multiple of the head count (window_attn_f16.hip), no more window ranges than windows / 8
  int gx = std::max(1, n_cu / nH);
  gx = std::min(gx, (B_ + WQ_WAVES - 1) / WQ_WAVES);
  const void* fn = reinterpret_cast<const void*>(&window_attn_qkv_f16x3<KS>);
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((window_attn_qkv_f16x3<KS>), dim3(gx * nH), dim3(64 * WQ_WAVES), lds, st, x, reinterpret_cast<const u32x4*>(wp), winv,
                     qkv_bias, bias, shift_mask, B_, nW, nH, gx, (int)xbytes, scale, out, wi, (65536 + wi.ws - 1) / wi.ws);
  return check_launch("window_attn_qkv_f16x3");
}

// x [B, H*W, C] in token order, (wp, winv) the split image of qkv.weight [3C, C]; out [B, H*W, C].  Returns 1 if launched, 0 if not
// covered, < 0 on error.
int window_attention_qkv_f16x3(const float* x, const void* wp, const float* winv, const float* qkv_bias, const float* bias,
                               const float* shift_mask, int B, int H, int W, int ws, int shift, int nH, int C, float scale, float* out,
                               hipStream_t st) {
  if (ws != 7 || (C != 96 && C != 192) || nH * WQ_HD != C) return 0;
  const long long xbytes = (long long)B * H * W * C * 4;
  if (xbytes >= 0x7FFFFFFFLL) return 0;                          // 32-bit byte offsets of x, 32-bit element offsets of out
  auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (mis(x, 16) || mis(wp, 16) || mis(winv, 4) || mis(qkv_bias, 4) || mis(bias, 4) || mis(shift_mask, 4) || mis(out, 4)) return 0;
  const WinImage wi = win_image(H, W, ws, shift);
  const int nW = (wi.Hp / ws) * wi.nWx;
  const int B_ = B * nW;
  if (B_ == 0) return 1;
  const int n_cu = cu_count();
  const int rc = C == 96 ? launch_wq<3>(x, wp, winv, qkv_bias, bias, shift_mask, B_, nW, nH, xbytes, scale, out, wi, n_cu, st)
                         : launch_wq<6>(x, wp, winv, qkv_bias, bias, shift_mask, B_, nW, nH, xbytes, scale, out, wi, n_cu, st);
  return rc == UNIVS_OK ? 1 : rc;
}

}  // namespace univs
