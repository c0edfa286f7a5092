// y[M, N] = act((x [+ xadd]) W^T + b) [+ residual] [-> LayerNorm] for FEW rows (M <= a few thousand): the per-token Linears of the
// UniVS decoder on its Q' T = 500 ... 2 000 query tokens (univs/modeling/transformer_decoder/transformer_layers.py: the in / out
// projections of SelfAttentionLayer :30-46 and CrossAttentionLayer :95-115, FFNLayer :150-166, the mask-embedding MLP :205-217).
// The library runs each of them as a tuned GEMM of 8 - 13 us (launch- and latency-bound: 33 MFLOP) with the elementwise steps around
// it -- `tgt + query_pos` in front, `norm(tgt + .)` behind -- as launches of their own: ~100 GEMMs + ~60 elementwise / LayerNorm
// launches per clip.
//
// Arithmetic: the three-product fp16 scheme of linear_f16x3.hip (two fp16 parts per operand behind power-of-two row scales, three
// v_mfma_f32_16x16x32_f16 per fp32 product, fp32 accumulation: ~2^-22 per product); W pre-split once per weight tensor
// (gemm_f16x3_stream.hip: presplit_f16x3, the layout [(k/8) * 2 + part][feature] of 16-byte units), x split on the fly.
// Organisation: everything here is latency and co-residency: a workgroup = 8 waves = 16 rows x 256 features (32 per wave: two MFMA
// feature blocks).  The 16 x K tile of the operand is staged ONCE per workgroup: every thread loads one 8-value slot (+ x_add),
// the row maxima meet in LDS (atomic max on the magnitude bits), the slot is scaled, split into its two fp16 parts and written to
// LDS in B-fragment order -- a wave then reads its operand with two ds_read_b128 per k-step instead of holding a private copy of
// the tile (64 registers: with 256 registers per lane a workgroup filled a CU's register file, so every launch had to wait for the
// CU to drain: 12.3 us per call in the trace against 8.5 for the library GEMM).  The A fragments come straight from the pre-split
// image in global memory (L2-resident: the same 256 KB for every workgroup), four 16-byte loads per k-step and lane, SL_AHEAD
// k-steps ahead; the epilogue's operands are requested up front.  Epilogue: bias, ReLU, residual, and -- when the workgroup holds
// whole rows (N == 256) -- nn.LayerNorm with exact two-pass statistics across the eight waves (two LDS exchanges).
#include "common.h"
#include "f16x3.h"
#include "launchers.h"
#include "xattn_merge.h"

#include <algorithm>
#include <cstdlib>

namespace univs {

constexpr int SL_WAVES = 8;
constexpr int SL_AHEAD = 4;     // k-steps of A fragments in flight
constexpr int SL_KMAX = 256;     // one 8-value slot of the operand tile per thread

struct SlArgs {
  const float* X;       // [M, K]
  const float* Xadd;    // [M, K] or null: the operand is X + Xadd (`with_pos_embed`)
  const u32x4* Wp;      // pre-split W [Nw, K]: unit ((k / 8) * 2 + part) * Nw + feature
  const float* winv;    // [Nw]
  const float* bias;    // [Nw] or null
  const float* Res;     // [M, N] or null
  const float* ln_g;    // [N] or null (then N == 256)
  const float* ln_b;    // [N] or null
  float ln_eps;
  float* Y;             // [M, N]
  int M, N, K, Nw, f_off, relu;   // features [f_off, f_off + N) of the pre-split matrix
  int out_T;                      // > 0: rows are (q, t) pairs, q-major with T = out_T; row (q, t) of the result is stored at (t, q) -- the
                                  // mask embeddings [Q', T, C] handed on as [T, Q', C] (...decoder_univs.py:527) without a copy of its own
  int add_features;               // Xadd applies to output features < add_features only (a multiple of 32; 0: to all) -- q, k = in_proj(tgt +
                                  // pos) and v = in_proj(tgt) of a self-attention in one launch
  // MERGE: the operand is the attention output [L, Nb, 32 Hh] (row = q * Nb + n), never written: a slot's eight values are merged from
  // the key segments' partials in `ws` (cross_attn.hip: [chunk][Nb * Hh][nseg][Lp][XA_PART]) while the tile is staged; X is unused
  const float* ws;
  int nseg, Lp, Nb, Hh;
};

typedef unsigned sl_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float sl_row_sum(float v) {          // over the four lanes (lane >> 4) that hold one row
  const sl_u2 s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float r1 = __uint_as_float(s1.x) + __uint_as_float(s1.y);
  const sl_u2 s2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(r1), __float_as_uint(r1), false, false);
  return __uint_as_float(s2.x) + __uint_as_float(s2.y);
}

template <bool MERGE>
__global__ __launch_bounds__(64 * SL_WAVES, MERGE ? 2 : 3) void small_linear_kernel(const SlArgs a) {
  // LDS: operand tiles [tile: with x_add / plain][part h, m][k-step][lane] 16-byte units | row maxima [2][16] | inverse scales [2][16]
  extern __shared__ __attribute__((aligned(16))) u32x4 xs[];
  __shared__ float red[2][SL_WAVES][16];
  __shared__ unsigned rmax[2][16];
  __shared__ float rinv[2][16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int M = a.M, N = a.N, K = a.K, KS = K >> 5;
  const int row0 = blockIdx.x * 16;
  const int fbase = blockIdx.y * (32 * SL_WAVES);
  const int f0 = fbase + wave * 32;                             // this wave's 32 features (within [0, N))
  const bool with_ln = a.ln_g != nullptr;                      // uniform; then N == 256 and every wave has features
  const bool f_ok1 = f0 + 16 < N;                               // second feature block inside N (N % 16 == 0)
  // which operand tiles this workgroup's waves read (uniform): tile 0 = x + x_add, tile 1 = x
  const int fend = min(fbase + 32 * SL_WAVES, N);
  const bool need_add = a.Xadd != nullptr && (a.add_features == 0 || fbase < a.add_features);
  const bool need_plain = a.Xadd == nullptr || (a.add_features != 0 && fend > a.add_features);
  const int my_tile = (a.Xadd != nullptr && (a.add_features == 0 || f0 < a.add_features)) ? 0 : 1;   // wave-uniform
  const int tile_units = 2 * KS * 64;

  // ---- A fragments: units ((4 ks + g) * 2 + part) * Nw + f_off + f0 + 16 q + j; the first SL_AHEAD k-steps are requested now
  const u32x4* wl = a.Wp + (size_t)(g * 2) * a.Nw + a.f_off + min(f0, N - 16) + j;
  const size_t kstep_units = (size_t)8 * a.Nw;
  u32x4 afr[SL_AHEAD][2][2];                                    // [stage][feature block][part]
  auto load_a = [&](int ks, u32x4 (&d)[2][2]) __attribute__((always_inline)) {
    const u32x4* p = wl + (size_t)ks * kstep_units;
    d[0][0] = p[0];
    d[0][1] = p[a.Nw];
    d[1][0] = f_ok1 ? p[16] : p[0];
    d[1][1] = f_ok1 ? p[a.Nw + 16] : p[a.Nw];
  };
#pragma unroll
  for (int u = 0; u < SL_AHEAD; ++u)
    if (u < KS) load_a(u, afr[u]);

  // ---- the operand tile(s): slot s = ks * 64 + (g_ * 16 + j_) holds the 8 values of row j_ at columns 32 ks + 8 g_
  if (tid < 32) (&rmax[0][0])[tid] = 0u;
  __syncthreads();
  constexpr int SLOTS = (SL_KMAX / 32) * 64 / (64 * SL_WAVES);  // per thread (1)
  f32x4 xw[SLOTS][2], xv[SLOTS][2];                            // (in this order: the other one gives small_linear_kernel<false> other registers)
#pragma unroll
  for (int i = 0; i < SLOTS; ++i) {
    const int s_ = tid + 64 * SL_WAVES * i;
    if (s_ < KS * 64) {
      const int ks = s_ >> 6, l_ = s_ & 63, j_ = l_ & 15, g_ = l_ >> 4;
      const long long off = (long long)min(row0 + j_, M - 1) * K + 32 * ks + 8 * g_;
      if constexpr (MERGE) {
        // row r = (query q, batch entry n), k-step = head, k-group = channels 8 g_ ...: rows past M repeat the last row, rows q >= L
        // of a chunk are never read
        const int r = min(row0 + j_, M - 1), q = r / a.Nb, n = r - q * a.Nb;
        const int chunk = q / a.Lp, ql = q - chunk * a.Lp;
        const float* base = a.ws + ((((long long)chunk * a.Nb * a.Hh + (n * a.Hh + ks)) * a.nseg) * a.Lp + ql) * XA_PART;
        float mv[8];
        xa_merge_partials<8>(base, (long long)a.Lp * XA_PART, a.nseg, 8 * g_, mv);
        xv[i][0] = (f32x4){mv[0], mv[1], mv[2], mv[3]};
        xv[i][1] = (f32x4){mv[4], mv[5], mv[6], mv[7]};
      } else {
        xv[i][0] = *reinterpret_cast<const f32x4*>(a.X + off);
        xv[i][1] = *reinterpret_cast<const f32x4*>(a.X + off + 4);
      }
      if (need_add) {
        xw[i][0] = xv[i][0] + *reinterpret_cast<const f32x4*>(a.Xadd + off);
        xw[i][1] = xv[i][1] + *reinterpret_cast<const f32x4*>(a.Xadd + off + 4);
        atomicMax(&rmax[0][j_], l3_absmax8(xw[i][0], xw[i][1]));
      }
      if (need_plain) atomicMax(&rmax[1][j_], l3_absmax8(xv[i][0], xv[i][1]));
    }
  }
  __syncthreads();                                              // the row maxima are complete
#pragma unroll
  for (int i = 0; i < SLOTS; ++i) {
    const int s_ = tid + 64 * SL_WAVES * i;
    if (s_ < KS * 64) {
      const int j_ = s_ & 15;
      float sc, inv;
      f16x8 h8, m8;
      if (need_add) {
        l3_scale(rmax[0][j_], 14, sc, inv);
        l3_split8(xw[i][0], xw[i][1], sc, h8, m8);
        xs[s_] = __builtin_bit_cast(u32x4, h8);
        xs[KS * 64 + s_] = __builtin_bit_cast(u32x4, m8);
        if (s_ < 16) rinv[0][s_] = inv;                          // (slot s_ < 16: k-step 0, g_ 0, row s_)
      }
      if (need_plain) {
        l3_scale(rmax[1][j_], 14, sc, inv);
        l3_split8(xv[i][0], xv[i][1], sc, h8, m8);
        xs[tile_units + s_] = __builtin_bit_cast(u32x4, h8);
        xs[tile_units + KS * 64 + s_] = __builtin_bit_cast(u32x4, m8);
        if (s_ < 16) rinv[1][s_] = inv;
      }
    }
  }
  __syncthreads();                                              // the tiles are in place
  if (f0 >= N && !with_ln) return;                              // (no barrier below without the LayerNorm)
  const float sx_inv = rinv[my_tile][j];
  // the epilogue's operands, requested ahead of the product
  const int m = min(row0 + j, M - 1);
  const int row = row0 + j;
  const bool row_ok = row < M;
  f32x4 e_wi[2], e_bi[2], e_res[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int f = f0 + 16 * q + 4 * g;
    const bool ok = f < N;                                      // (N % 4 == 0)
    const int fw = a.f_off + (ok ? f : 0);
    e_wi[q] = *reinterpret_cast<const f32x4*>(a.winv + fw);
    e_bi[q] = a.bias ? *reinterpret_cast<const f32x4*>(a.bias + fw) : (f32x4){0.f, 0.f, 0.f, 0.f};
    e_res[q] = (a.Res && ok) ? *reinterpret_cast<const f32x4*>(a.Res + (long long)m * N + f) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const u32x4* xt = xs + my_tile * tile_units + lane;

  // ---- the product
  f32x4 acc[2][1];                                              // [block][the one column tile]: l3_mfma3_pair's form
  acc[0][0] = acc[1][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int kb = 0; kb < KS; kb += SL_AHEAD) {
#pragma unroll
    for (int u = 0; u < SL_AHEAD; ++u) {
      const int ks = kb + u;
      if (ks < KS) {                                            // uniform
        const f16x8 bh[1] = {__builtin_bit_cast(f16x8, xt[ks * 64])}, bm[1] = {__builtin_bit_cast(f16x8, xt[KS * 64 + ks * 64])};
        l3_mfma3_pair<1>(afr[u], bh, bm, acc[0], acc[1]);
        __builtin_amdgcn_sched_barrier(0);                       // (the refill below overwrites the fragments just consumed: no copies)
        if (ks + SL_AHEAD < KS) load_a(ks + SL_AHEAD, afr[u]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }

  // ---- epilogue: D[i = feature][j = row]: a lane holds features f0 + 16 q + 4 g ... + 3 of row j
  f32x4 v[2];
  float sm = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int f = f0 + 16 * q + 4 * g;
    const bool ok = f < N;
    f32x4 t = (acc[q][0] * sx_inv) * e_wi[q] + e_bi[q];
    if (a.relu) t = __builtin_elementwise_maximum(t, (f32x4){0.f, 0.f, 0.f, 0.f});   // NaN-propagating, as torch.relu
    t += e_res[q];
    v[q] = ok ? t : (f32x4){0.f, 0.f, 0.f, 0.f};
    sm += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
  }
  if (with_ln) {
    // nn.LayerNorm over the row's 256 values: 8 in this lane, 32 in this wave (its four lanes of the row), the rest in the other waves
    const float inv_n = 1.0f / (float)N;
    const float ws = sl_row_sum(sm);
    if (g == 0) red[0][wave][j] = ws;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < SL_WAVES; ++w) tot += red[0][w][j];
    const float mean = tot * inv_n;
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      v[q] -= mean;
#pragma unroll
      for (int e = 0; e < 4; ++e) sq = fmaf(v[q][e], v[q][e], sq);
    }
    const float wq = sl_row_sum(sq);
    if (g == 0) red[1][wave][j] = wq;
    __syncthreads();
    float tq = 0.f;
#pragma unroll
    for (int w = 0; w < SL_WAVES; ++w) tq += red[1][w][j];
    const float rstd = 1.0f / sqrtf(tq * inv_n + a.ln_eps);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = f0 + 16 * q + 4 * g;
      const f32x4 gm = *reinterpret_cast<const f32x4*>(a.ln_g + f);
      f32x4 y = (v[q] * rstd) * gm;
      if (a.ln_b) y += *reinterpret_cast<const f32x4*>(a.ln_b + f);
      v[q] = y;
    }
  }
  const int orow = a.out_T > 0 ? (row % a.out_T) * (M / a.out_T) + row / a.out_T : row;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int f = f0 + 16 * q + 4 * g;
    if (row_ok && f < N) *reinterpret_cast<f32x4*>(a.Y + (long long)orow * N + f) = v[q];
  }
}

// returns UNIVS_OK, or UNIVS_ERR_NOT_IMPLEMENTED when the shape is not covered
int small_linear_f32(const float* x, const float* xadd, const void* wp, const float* winv, const float* bias, int n_w, int f_off,
                     const float* residual, const float* ln_g, const float* ln_b, float ln_eps, float* y, long long M, int N, int K,
                     int relu, int add_features, int out_T, hipStream_t st) {
  if (M <= 0 || N <= 0) return UNIVS_OK;
  auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  if (K < 32 || K % 32 != 0 || K > SL_KMAX || N % 16 != 0 || n_w % 4 != 0 || f_off % 4 != 0 || f_off < 0 || f_off + N > n_w || M > 16LL * 65535 ||
      (ln_g && N != 32 * SL_WAVES) || (ln_b && !ln_g) || add_features < 0 || add_features % 32 != 0 || out_T < 0 || (out_T > 0 && (M % out_T != 0 || residual || ln_g)) || mis(x) || mis(xadd) || mis(wp) || mis(winv) || mis(bias) || mis(residual) ||
      mis(ln_g) || mis(ln_b) || mis(y) || M * (long long)std::max(N, K) * 4 >= 0x7FFFFFFFLL)
    return UNIVS_ERR_NOT_IMPLEMENTED;
  SlArgs a{};
  a.X = x; a.Xadd = xadd; a.Wp = reinterpret_cast<const u32x4*>(wp); a.winv = winv; a.bias = bias; a.Res = residual;
  a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = ln_eps; a.Y = y;
  a.M = (int)M; a.N = N; a.K = K; a.Nw = n_w; a.f_off = f_off; a.relu = relu ? 1 : 0; a.add_features = add_features; a.out_T = out_T;
  dim3 grid((unsigned)((M + 15) / 16), (unsigned)((N + 32 * SL_WAVES - 1) / (32 * SL_WAVES)));
  const size_t lds = (size_t)2 * 2 * (K / 32) * 64 * 16;        // two operand tiles (x + x_add, x), two parts each
  hipLaunchKernelGGL(small_linear_kernel<false>, grid, dim3(64 * SL_WAVES), lds, st, a);
  return check_launch("small_linear_f32");
}

// The same Linear on the attention output [L, Nb, 32 Hh] that is merged from the partials in `ws` while the operand tile is staged
// (`plan` = segments + 65536 x query blocks per wave, as cross_attention_partials_f32 reported it): no xattn_merge launch, no
// [L, Nb, E] tensor.  Bit-identical to small_linear_f32 on xattn_merge's output.  Returns as small_linear_f32.
int small_linear_merged_f32(const float* ws, int plan, int L, int Nb, int Hh, const void* wp, const float* winv, const float* bias, int n_w,
                            int f_off, const float* residual, const float* ln_g, const float* ln_b, float ln_eps, float* y, int N,
                            hipStream_t st) {
  const long long M = (long long)L * Nb;
  if (M <= 0 || N <= 0) return UNIVS_OK;
  auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  const int nseg = plan & 0xffff, nqb = plan >> 16, K = 32 * Hh;
  if (nseg < 1 || nqb < 1 || nqb > 7 || Hh < 1 || K > SL_KMAX || N % 16 != 0 || n_w % 4 != 0 || f_off % 4 != 0 || f_off < 0 || f_off + N > n_w ||
      M > 16LL * 65535 || (ln_g && N != 32 * SL_WAVES) || (ln_b && !ln_g) || (reinterpret_cast<uintptr_t>(ws) & 7) || mis(wp) || mis(winv) ||
      mis(bias) || mis(residual) || mis(ln_g) || mis(ln_b) || mis(y) || M * (long long)std::max(N, K) * 4 >= 0x7FFFFFFFLL)
    return UNIVS_ERR_NOT_IMPLEMENTED;
  SlArgs a{};
  a.X = nullptr; a.Xadd = nullptr; a.Wp = reinterpret_cast<const u32x4*>(wp); a.winv = winv; a.bias = bias; a.Res = residual;
  a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = ln_eps; a.Y = y;
  a.M = (int)M; a.N = N; a.K = K; a.Nw = n_w; a.f_off = f_off; a.relu = 0; a.add_features = 0; a.out_T = 0;
  a.ws = ws; a.nseg = nseg; a.Lp = 16 * nqb; a.Nb = Nb; a.Hh = Hh;
  dim3 grid((unsigned)((M + 15) / 16), (unsigned)((N + 32 * SL_WAVES - 1) / (32 * SL_WAVES)));
  const size_t lds = (size_t)2 * 2 * (K / 32) * 64 * 16;
  hipLaunchKernelGGL(small_linear_kernel<true>, grid, dim3(64 * SL_WAVES), lds, st, a);
  return check_launch("small_linear_merged_f32");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// A CHAIN of up to three 256 -> 256 Linears on few rows in ONE launch: y = L3(act(L2(act(L1(LN?(x)))))) -- the mask-embedding MLP of every
// prediction head (univs/modeling/transformer_decoder/transformer_layers.py:205-217 `MLP`, called at ...decoder_univs.py:520 on the
// `decoder_norm`-ed queries): three launches of small_linear_kernel (8 us each, all of it launch ramp and latency) and a LayerNorm launch
// per head, ten heads per clip.  Same workgroup shape (8 waves = 16 rows x 256 features) and the same arithmetic; between two stages the
// 16 x 256 result goes back to LDS AS THE NEXT OPERAND: every lane holds 2 x 4 consecutive features of one row, the row maxima meet in
// LDS (atomic max), the lane scales, splits and writes its two 8-byte halves of the B-fragment units -- the values, the row maximum, the
// scale and the parts are what the next launch would have read back from memory and computed, so the chain is bit-identical to the
// sequence of launches.  The next stage's first weight fragments are requested before the two barriers of the hand-over.
// Optional nn.LayerNorm on the INPUT rows (`decoder_norm`): exact two-pass statistics over the staged tile, summed in a fixed order.
struct SlChainArgs {
  const float* X;       // [M, 256]
  const u32x4* Wp[3];   // pre-split W_s [256, 256]
  const float* winv[3];
  const float* bias[3];
  int relu[3];
  int stages;
  const float* in_g;    // LayerNorm on x (weight / bias / eps) or null
  const float* in_b;
  float in_eps;
  float* Xn;            // [M, 256] or null: the normalised input rows (for the callers that need `decoder_norm(x)` itself)
  float* Y;             // [M, 256] (out_T > 0: row (q, t) stored at (t, q))
  int M, out_T;
  // the end of a decoder layer in front of the chain (both optional):
  // PRE: the rows are x = LayerNorm(X + pre_res) -- the FFN's `norm(tgt + linear2(.))` on the library GEMM's output X --, stored to Xr (the
  // layer's output); statistics and expressions of layer_norm_f32_kernel<64, 1, true, false> (layer_norm.hip), in its summation order
  const float* pre_res; // [M, 256] or null
  const float* pre_g;   // [256]
  const float* pre_b;   // [256]
  float pre_eps;
  float* Xr;            // [M, 256]
  // SIDE: side_Y = (x + side_add) W_side^T + b_side from the rows x as loaded (after PRE, before the input LayerNorm) -- the next layer's
  // cross-attention query projection --, a stage of its own in front of the chain: own row maxima, own operand tile
  const float* side_add;   // [M, 256] or null
  const u32x4* side_Wp;    // pre-split [side_Nw, 256] or null (no side stage): its features [side_f_off, side_f_off + 256)
  const float* side_winv;  // [side_Nw]
  const float* side_bias;  // [side_Nw] or null
  float* side_Y;           // [M, 256]
  int side_Nw, side_f_off;
};

// layer_norm_f32_kernel<64, 1, ...>'s row sum at this workgroup's shape: that kernel holds a row's 64 four-value chunks in the 64 lanes of
// a wave and adds them with an xor butterfly (32, 16, ..., 1); here thread (wave ks, g_, j_) holds chunks 8 ks + 2 g_ and + 1 of row j_.
// The chunk values go through LDS, wave w replays the butterfly for rows 2 w and 2 w + 1, and every thread reads its row's total.
__device__ __forceinline__ float sl_ln_row_total(float c0, float c1, float (&part)[16][64], float (&total)[16], int wave, int lane, int chunk,
                                                 int j_) {
  part[j_][chunk] = c0;
  part[j_][chunk + 1] = c1;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    float v = part[2 * wave + r][lane];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) total[2 * wave + r] = v;
  }
  __syncthreads();
  return total[j_];
}

__global__ __launch_bounds__(64 * SL_WAVES, 3) void small_chain_kernel(const SlChainArgs a) {
  constexpr int K = 256, N = 256, KS = K >> 5;
  __shared__ __attribute__((aligned(16))) u32x4 xs[2][2 * KS * 64];      // two operand tiles (ping-pong), [part][k-step][lane]
  __shared__ unsigned rmax[4][16];                                        // the chain's stages | the side stage
  __shared__ float rstat[2][SL_WAVES][16];
  __shared__ float pre_part[16][64], pre_total[16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int M = a.M;
  const int row0 = blockIdx.x * 16;
  const int f0 = wave * 32;
  const bool side = a.side_Wp != nullptr;                                 // uniform

  u32x4 afr[SL_AHEAD][2][2];
  auto load_a = [&](const u32x4* wl, int ks, u32x4 (&d)[2][2]) __attribute__((always_inline)) {
    const u32x4* p = wl + (size_t)ks * (8 * N);
    d[0][0] = p[0];
    d[0][1] = p[N];
    d[1][0] = p[16];
    d[1][1] = p[N + 16];
  };
  const size_t wl_off = (size_t)(g * 2) * N + f0 + j;
  // (the side stage's features are a range of a packed image: its own strides)
  const u32x4* wl_side = a.side_Wp + (size_t)(g * 2) * a.side_Nw + a.side_f_off + f0 + j;
  auto load_side = [&](int ks, u32x4 (&d)[2][2]) __attribute__((always_inline)) {
    const u32x4* p = wl_side + (size_t)ks * (8 * (size_t)a.side_Nw);
    d[0][0] = p[0];
    d[0][1] = p[a.side_Nw];
    d[1][0] = p[16];
    d[1][1] = p[a.side_Nw + 16];
  };
  if (side) {
#pragma unroll
    for (int u = 0; u < SL_AHEAD; ++u) load_side(u, afr[u]);
  } else {
#pragma unroll
    for (int u = 0; u < SL_AHEAD; ++u) load_a(a.Wp[0] + wl_off, u, afr[u]);
  }

  if (tid < 64) (&rmax[0][0])[tid] = 0u;
  __syncthreads();
  // ---- stage-0 operand: slot s_ = tid (KS * 64 = 512 slots): row j_ = s_ & 15, columns 32 ks + 8 g_
  {
    const int s_ = tid;
    const int ks = s_ >> 6, l_ = s_ & 63, j_ = l_ & 15, g_ = l_ >> 4;
    const int mrow = min(row0 + j_, M - 1);
    const long long off = (long long)mrow * K + 32 * ks + 8 * g_;
    f32x4 x0 = *reinterpret_cast<const f32x4*>(a.X + off), x1 = *reinterpret_cast<const f32x4*>(a.X + off + 4);
    f32x4 w0, w1;
    if (side && a.side_add) {                                     // (requested ahead of PRE's exchanges)
      w0 = *reinterpret_cast<const f32x4*>(a.side_add + off);
      w1 = *reinterpret_cast<const f32x4*>(a.side_add + off + 4);
    } else {
      w0 = w1 = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (a.pre_res) {
#pragma clang fp contract(off)                                    // layer_norm_f32_kernel's operations as hipcc compiled them, spelled out
      const int c = 32 * ks + 8 * g_;
      const f32x4 pg0 = *reinterpret_cast<const f32x4*>(a.pre_g + c), pg1 = *reinterpret_cast<const f32x4*>(a.pre_g + c + 4);
      const f32x4 pb0 = *reinterpret_cast<const f32x4*>(a.pre_b + c), pb1 = *reinterpret_cast<const f32x4*>(a.pre_b + c + 4);
      x0 += *reinterpret_cast<const f32x4*>(a.pre_res + off);
      x1 += *reinterpret_cast<const f32x4*>(a.pre_res + off + 4);
      const float tot = sl_ln_row_total(0.f + ((x0[0] + x0[1]) + (x0[2] + x0[3])), 0.f + ((x1[0] + x1[1]) + (x1[2] + x1[3])), pre_part,
                                        pre_total, wave, lane, 8 * ks + 2 * g_, j_);
      const float mean = tot / (float)K;
      x0 -= mean;
      x1 -= mean;
      const float tq = sl_ln_row_total(fmaf(x0[0], x0[0], x0[1] * x0[1]) + fmaf(x0[2], x0[2], x0[3] * x0[3]),
                                       fmaf(x1[0], x1[0], x1[1] * x1[1]) + fmaf(x1[2], x1[2], x1[3] * x1[3]), pre_part, pre_total, wave, lane,
                                       8 * ks + 2 * g_, j_);
      const float rstd = 1.f / sqrtf(fmaf(1.f / (float)K, tq, a.pre_eps));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x0[e] = fmaf(x0[e] * rstd, pg0[e], pb0[e]);
        x1[e] = fmaf(x1[e] * rstd, pg1[e], pb1[e]);
      }
      if (row0 + j_ < M) {
        *reinterpret_cast<f32x4*>(a.Xr + off) = x0;
        *reinterpret_cast<f32x4*>(a.Xr + off + 4) = x1;
      }
    }
    if (side) {
      w0 += x0;
      w1 += x1;
      atomicMax(&rmax[3][j_], l3_absmax8(w0, w1));
    }
    if (a.in_g) {
      // nn.LayerNorm over the row: mean, then the centred second moment (two passes).  A row's 32 slots sit in the four lanes j_ + 16 g_
      // of each of the 8 waves: lane sums by permlane swaps, wave sums through LDS, added in a fixed order (deterministic)
      const float s4 = sl_row_sum(((x0[0] + x0[1]) + (x0[2] + x0[3])) + ((x1[0] + x1[1]) + (x1[2] + x1[3])));
      if (g_ == 0) rstat[0][ks][j_] = s4;
      __syncthreads();
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < SL_WAVES; ++w) tot += rstat[0][w][j_];
      const float mean = tot * (1.0f / K);
      x0 -= mean;
      x1 -= mean;
      float sq = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) sq = fmaf(x0[e], x0[e], fmaf(x1[e], x1[e], sq));
      const float q4 = sl_row_sum(sq);
      if (g_ == 0) rstat[1][ks][j_] = q4;
      __syncthreads();
      float tq = 0.f;
#pragma unroll
      for (int w = 0; w < SL_WAVES; ++w) tq += rstat[1][w][j_];
      const float rstd = 1.0f / sqrtf(tq * (1.0f / K) + a.in_eps);
      const int c = 32 * ks + 8 * g_;
      x0 = (x0 * rstd) * *reinterpret_cast<const f32x4*>(a.in_g + c);
      x1 = (x1 * rstd) * *reinterpret_cast<const f32x4*>(a.in_g + c + 4);
      if (a.in_b) {
        x0 += *reinterpret_cast<const f32x4*>(a.in_b + c);
        x1 += *reinterpret_cast<const f32x4*>(a.in_b + c + 4);
      }
      if (a.Xn && row0 + j_ < M) {
        *reinterpret_cast<f32x4*>(a.Xn + off) = x0;
        *reinterpret_cast<f32x4*>(a.Xn + off + 4) = x1;
      }
    }
    atomicMax(&rmax[0][j_], l3_absmax8(x0, x1));
    __syncthreads();
    float sc, inv;
    l3_scale(rmax[0][j_], 14, sc, inv);
    f16x8 h8, m8;
    l3_split8(x0, x1, sc, h8, m8);
    xs[0][s_] = __builtin_bit_cast(u32x4, h8);
    xs[0][KS * 64 + s_] = __builtin_bit_cast(u32x4, m8);
    if (side) {
      l3_scale(rmax[3][j_], 14, sc, inv);
      l3_split8(w0, w1, sc, h8, m8);
      xs[1][s_] = __builtin_bit_cast(u32x4, h8);
      xs[1][KS * 64 + s_] = __builtin_bit_cast(u32x4, m8);
    }
  }
  __syncthreads();

  const int row = row0 + j;
  const bool row_ok = row < M;
  f32x4 v[2];
  if (side) {
    // the side stage: a small_linear_kernel product on its tile (xs[1]: the chain's first hand-over writes there behind a barrier)
    float sc_, sx_inv;
    l3_scale(rmax[3][j], 14, sc_, sx_inv);
    const u32x4* xt = xs[1] + lane;
    f32x4 e_wi[2], e_bi[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = a.side_f_off + f0 + 16 * q + 4 * g;
      e_wi[q] = *reinterpret_cast<const f32x4*>(a.side_winv + f);
      e_bi[q] = a.side_bias ? *reinterpret_cast<const f32x4*>(a.side_bias + f) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    f32x4 acc[2][1];
    acc[0][0] = acc[1][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KS; kb += SL_AHEAD) {
#pragma unroll
      for (int u = 0; u < SL_AHEAD; ++u) {
        const int ks = kb + u;
        const f16x8 bh[1] = {__builtin_bit_cast(f16x8, xt[ks * 64])}, bm[1] = {__builtin_bit_cast(f16x8, xt[KS * 64 + ks * 64])};
        l3_mfma3_pair<1>(afr[u], bh, bm, acc[0], acc[1]);
        __builtin_amdgcn_sched_barrier(0);
        if (ks + SL_AHEAD < KS) load_side(ks + SL_AHEAD, afr[u]);
        else load_a(a.Wp[0] + wl_off, ks + SL_AHEAD - KS, afr[u]);              // the chain's first fragments
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f32x4 t = (acc[q][0] * sx_inv) * e_wi[q] + e_bi[q];
      t += (f32x4){0.f, 0.f, 0.f, 0.f};                          // (small_linear_kernel's `+ residual` without one: -0 -> +0)
      if (row_ok) *reinterpret_cast<f32x4*>(a.side_Y + (long long)row * N + f0 + 16 * q + 4 * g) = t;
    }
  }
#pragma unroll 1
  for (int st = 0; st < a.stages; ++st) {
    float sc_, sx_inv;
    l3_scale(rmax[st][j], 14, sc_, sx_inv);
    const u32x4* xt = xs[st & 1] + lane;
    const u32x4* wl = a.Wp[st] + wl_off;
    f32x4 e_wi[2], e_bi[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = f0 + 16 * q + 4 * g;
      e_wi[q] = *reinterpret_cast<const f32x4*>(a.winv[st] + f);
      e_bi[q] = a.bias[st] ? *reinterpret_cast<const f32x4*>(a.bias[st] + f) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    f32x4 acc[2][1];
    acc[0][0] = acc[1][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KS; kb += SL_AHEAD) {
#pragma unroll
      for (int u = 0; u < SL_AHEAD; ++u) {
        const int ks = kb + u;
        const f16x8 bh[1] = {__builtin_bit_cast(f16x8, xt[ks * 64])}, bm[1] = {__builtin_bit_cast(f16x8, xt[KS * 64 + ks * 64])};
        l3_mfma3_pair<1>(afr[u], bh, bm, acc[0], acc[1]);
        __builtin_amdgcn_sched_barrier(0);
        if (ks + SL_AHEAD < KS) load_a(wl, ks + SL_AHEAD, afr[u]);
        else if (st + 1 < a.stages) load_a(a.Wp[st + 1] + wl_off, ks + SL_AHEAD - KS, afr[u]);   // the next stage's first fragments
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f32x4 t = (acc[q][0] * sx_inv) * e_wi[q] + e_bi[q];
      if (a.relu[st]) t = __builtin_elementwise_maximum(t, (f32x4){0.f, 0.f, 0.f, 0.f});
      v[q] = t;
    }
    if (st + 1 < a.stages) {
      // hand-over: the result rows become the next operand tile (see the header)
      atomicMax(&rmax[st + 1][j], l3_absmax8(v[0], v[1]));
      __syncthreads();
      float sc, inv;
      l3_scale(rmax[st + 1][j], 14, sc, inv);
      _Float16* dst = reinterpret_cast<_Float16*>(xs[(st + 1) & 1]);
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        h4 hh, mm;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xsv = v[q][e] * sc;
          hh[e] = (_Float16)xsv;
          mm[e] = (_Float16)(xsv - (float)hh[e]);
        }
        const int unit = wave * 64 + (2 * q + (g >> 1)) * 16 + j;           // k-step = this wave's 32 features
        *reinterpret_cast<h4*>(dst + (size_t)unit * 8 + 4 * (g & 1)) = hh;
        *reinterpret_cast<h4*>(dst + (size_t)(KS * 64 + unit) * 8 + 4 * (g & 1)) = mm;
      }
      __syncthreads();
    }
  }
  const int orow = a.out_T > 0 ? (row % a.out_T) * (M / a.out_T) + row / a.out_T : row;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int f = f0 + 16 * q + 4 * g;
    if (row_ok) *reinterpret_cast<f32x4*>(a.Y + (long long)orow * N + f) = v[q];
  }
}

// `pre_*` / `xr` and `side_*`: the two optional stages in front of the chain (SlChainArgs); all NULL: the plain chain
int small_chain_seam_f32(const float* x, const float* pre_res, const float* pre_g, const float* pre_b, float pre_eps, float* xr,
                         const float* side_add, const void* side_wp, const float* side_winv, const float* side_bias, int side_nw,
                         int side_f_off, float* side_y, int stages, const void* const* wp, const float* const* winv,
                         const float* const* bias, const int* relu, const float* in_g, const float* in_b, float in_eps, float* xn, float* y,
                         long long M, int out_T, hipStream_t st) {
  if (M <= 0) return UNIVS_OK;
  auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  if (stages < 1 || stages > 3 || M > 16LL * 65535 || out_T < 0 || (out_T > 0 && M % out_T != 0) || mis(x) || mis(y) || mis(xn) || mis(in_g) ||
      mis(in_b) || (in_b && !in_g) || (xn && !in_g) || M * 256LL * 4 >= 0x7FFFFFFFLL)
    return UNIVS_ERR_NOT_IMPLEMENTED;
  if ((pre_res && (!pre_g || !pre_b || !xr)) || (!pre_res && (pre_g || pre_b || xr)) || mis(pre_res) || mis(pre_g) || mis(pre_b) || mis(xr) ||
      (side_wp && (!side_winv || !side_y || side_nw % 4 != 0 || side_f_off % 4 != 0 || side_f_off < 0 || side_f_off + 256 > side_nw)) ||
      (!side_wp && (side_add || side_winv || side_bias || side_y)) || mis(side_add) || mis(side_wp) ||
      mis(side_winv) || mis(side_bias) || mis(side_y))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  SlChainArgs a{};
  a.X = x; a.stages = stages; a.in_g = in_g; a.in_b = in_b; a.in_eps = in_eps; a.Xn = xn; a.Y = y; a.M = (int)M; a.out_T = out_T;
  a.pre_res = pre_res; a.pre_g = pre_g; a.pre_b = pre_b; a.pre_eps = pre_eps; a.Xr = xr;
  a.side_add = side_add; a.side_Wp = reinterpret_cast<const u32x4*>(side_wp); a.side_winv = side_winv; a.side_bias = side_bias; a.side_Y = side_y;
  a.side_Nw = side_nw; a.side_f_off = side_f_off;
  for (int s_ = 0; s_ < stages; ++s_) {
    if (!wp[s_] || !winv[s_] || mis(wp[s_]) || mis(winv[s_]) || mis(bias[s_])) return UNIVS_ERR_NOT_IMPLEMENTED;
    a.Wp[s_] = reinterpret_cast<const u32x4*>(wp[s_]); a.winv[s_] = winv[s_]; a.bias[s_] = bias[s_]; a.relu[s_] = relu[s_] ? 1 : 0;
  }
  hipLaunchKernelGGL(small_chain_kernel, dim3((unsigned)((M + 15) / 16)), dim3(64 * SL_WAVES), 0, st, a);
  return check_launch("small_chain_f32");
}

int small_chain_f32(const float* x, int stages, const void* const* wp, const float* const* winv, const float* const* bias, const int* relu,
                    const float* in_g, const float* in_b, float in_eps, float* xn, float* y, long long M, int out_T, hipStream_t st) {
  return small_chain_seam_f32(x, nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, stages, wp, winv,
                              bias, relu, in_g, in_b, in_eps, xn, y, M, out_T, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// A SEAM between two sub-layers of a post-norm decoder layer in ONE launch: t = LayerNorm(residual + x W_a^T + b_a) -- the tail of an
// attention sub-layer, exactly small_linear_kernel<false> with its residual + LayerNorm epilogue (K = N = 256) -- and
// y = act((t [+ add]) W_b^T + b_b), the first Linear of the NEXT sub-layer (the packed self-attention in-projection behind the
// cross-attention, the FFN's linear1 + ReLU behind the self-attention), which reads nothing but t.  t is stored (the next residual
// needs it) and handed over as small_chain_kernel hands a stage's rows over: the 16 x 256 rows of t [+ add, summed in fp32 registers]
// meet their row maxima in LDS, are scaled, split and written as stage B's operand tile(s) -- the values, maxima, scales and parts a
// separate launch would have loaded and computed, so both outputs have the bits of the two launches.  `add_features` as in SlArgs:
// two tiles (t + add for the output features below it, t for the rest), a workgroup builds only what its features read.
// Grid (row tiles, N_b / 256): every workgroup of a row tile recomputes stage A for its 16 rows (deterministic: the same bits in each),
// blockIdx.y == 0 stores t -- the column groups run side by side, not behind each other in one workgroup (all of this is latency).
struct SlSeamArgs {
  const float* X;       // [M, 256]: stage A's operand
  const u32x4* Wa;      // pre-split W_a [256, 256]
  const float* winv_a;  // [256]
  const float* bias_a;  // [256] or null
  const float* Res;     // [M, 256]
  const float* ln_g;    // [256]
  const float* ln_b;    // [256] or null
  float ln_eps;
  float* T;             // [M, 256]
  const float* Add;     // [M, 256] or null: stage B's operand is t + Add (`with_pos_embed`)
  const u32x4* Wb;      // pre-split W_b [Nwb, 256]
  const float* winv_b;  // [Nwb]
  const float* bias_b;  // [Nwb] or null
  float* Y;             // [M, Nb]
  int M, Nb, Nwb, f_off, relu, add_features;   // stage B: features [f_off, f_off + Nb) of W_b, Nb % 256 == 0
};

__global__ __launch_bounds__(64 * SL_WAVES, 3) void small_seam_kernel(const SlSeamArgs a) {
  constexpr int K = 256, N = 256, KS = K >> 5;
  __shared__ __attribute__((aligned(16))) u32x4 xs[2][2 * KS * 64];      // [0]: stage A's operand, then the plain t tile; [1]: the t + add tile
  __shared__ float red[2][SL_WAVES][16];
  __shared__ unsigned rmax[3][16];                                        // stage A's operand | t + add | t
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int M = a.M;
  const int row0 = blockIdx.x * 16;
  const int f0 = wave * 32;                                     // this wave's features of stage A = its k-step of stage B's operand
  const int fbase = blockIdx.y * N, fb0 = fbase + f0;           // its features of stage B (within [0, Nb))
  // which operand tiles this workgroup's waves read in stage B (uniform), as small_linear_kernel: tile 1 = t + add, tile 0 = t
  const bool need_add = a.Add != nullptr && (a.add_features == 0 || fbase < a.add_features);
  const bool need_plain = a.Add == nullptr || (a.add_features != 0 && fbase + N > a.add_features);
  const bool my_add = a.Add != nullptr && (a.add_features == 0 || fb0 < a.add_features);                 // wave-uniform

  u32x4 afr[SL_AHEAD][2][2];
  auto load_a = [&](const u32x4* wl, int nw, int ks, u32x4 (&d)[2][2]) __attribute__((always_inline)) {
    const u32x4* p = wl + (size_t)ks * (8 * (size_t)nw);
    d[0][0] = p[0];
    d[0][1] = p[nw];
    d[1][0] = p[16];
    d[1][1] = p[nw + 16];
  };
  const u32x4* wla = a.Wa + (size_t)(g * 2) * N + f0 + j;
  const u32x4* wlb = a.Wb + (size_t)(g * 2) * a.Nwb + a.f_off + fb0 + j;
#pragma unroll
  for (int u = 0; u < SL_AHEAD; ++u) load_a(wla, N, u, afr[u]);

  if (tid < 48) (&rmax[0][0])[tid] = 0u;
  __syncthreads();
  // ---- stage A's operand: slot s_ = tid: row j_ = s_ & 15, columns 32 ks + 8 g_ (small_linear_kernel's staging, one plain tile)
  {
    const int s_ = tid;
    const int ks = s_ >> 6, l_ = s_ & 63, j_ = l_ & 15, g_ = l_ >> 4;
    const long long off = (long long)min(row0 + j_, M - 1) * K + 32 * ks + 8 * g_;
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(a.X + off), x1 = *reinterpret_cast<const f32x4*>(a.X + off + 4);
    atomicMax(&rmax[0][j_], l3_absmax8(x0, x1));
    __syncthreads();
    float sc, inv;
    l3_scale(rmax[0][j_], 14, sc, inv);
    f16x8 h8, m8;
    l3_split8(x0, x1, sc, h8, m8);
    xs[0][s_] = __builtin_bit_cast(u32x4, h8);
    xs[0][KS * 64 + s_] = __builtin_bit_cast(u32x4, m8);
  }
  __syncthreads();

  const int m = min(row0 + j, M - 1);
  const int row = row0 + j;
  const bool row_ok = row < M;
  f32x4 v[2], w[2], eb_wi[2], eb_bi[2];                          // t, t + add, stage B's epilogue operands
  {
    float sc_, sx_inv;
    l3_scale(rmax[0][j], 14, sc_, sx_inv);
    f32x4 e_wi[2], e_bi[2], e_res[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = f0 + 16 * q + 4 * g;
      e_wi[q] = *reinterpret_cast<const f32x4*>(a.winv_a + f);
      e_bi[q] = a.bias_a ? *reinterpret_cast<const f32x4*>(a.bias_a + f) : (f32x4){0.f, 0.f, 0.f, 0.f};
      e_res[q] = *reinterpret_cast<const f32x4*>(a.Res + (long long)m * N + f);
    }
    const u32x4* xt = xs[0] + lane;
    f32x4 acc[2][1];
    acc[0][0] = acc[1][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KS; kb += SL_AHEAD) {
#pragma unroll
      for (int u = 0; u < SL_AHEAD; ++u) {
        const int ks = kb + u;
        const f16x8 bh[1] = {__builtin_bit_cast(f16x8, xt[ks * 64])}, bm[1] = {__builtin_bit_cast(f16x8, xt[KS * 64 + ks * 64])};
        l3_mfma3_pair<1>(afr[u], bh, bm, acc[0], acc[1]);
        __builtin_amdgcn_sched_barrier(0);
        if (ks + SL_AHEAD < KS) load_a(wla, N, ks + SL_AHEAD, afr[u]);
        else load_a(wlb, a.Nwb, ks + SL_AHEAD - KS, afr[u]);     // stage B's first fragments, ahead of the hand-over's barriers
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // what the hand-over and stage B's epilogue read, requested ahead of the LayerNorm's two exchanges
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = a.f_off + fb0 + 16 * q + 4 * g;
      eb_wi[q] = *reinterpret_cast<const f32x4*>(a.winv_b + f);
      eb_bi[q] = a.bias_b ? *reinterpret_cast<const f32x4*>(a.bias_b + f) : (f32x4){0.f, 0.f, 0.f, 0.f};
      w[q] = need_add ? *reinterpret_cast<const f32x4*>(a.Add + (long long)m * N + f0 + 16 * q + 4 * g) : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // the epilogue of small_linear_kernel with a residual and a LayerNorm, expression by expression
    float sm = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      f32x4 t = (acc[q][0] * sx_inv) * e_wi[q] + e_bi[q];
      t += e_res[q];
      v[q] = t;
      sm += (v[q][0] + v[q][1]) + (v[q][2] + v[q][3]);
    }
    const float inv_n = 1.0f / (float)N;
    const float ws = sl_row_sum(sm);
    if (g == 0) red[0][wave][j] = ws;
    __syncthreads();                                              // (every wave is done with stage A's tile here)
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < SL_WAVES; ++w) tot += red[0][w][j];
    const float mean = tot * inv_n;
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      v[q] -= mean;
#pragma unroll
      for (int e = 0; e < 4; ++e) sq = fmaf(v[q][e], v[q][e], sq);
    }
    const float wq = sl_row_sum(sq);
    if (g == 0) red[1][wave][j] = wq;
    __syncthreads();
    float tq = 0.f;
#pragma unroll
    for (int w = 0; w < SL_WAVES; ++w) tq += red[1][w][j];
    const float rstd = 1.0f / sqrtf(tq * inv_n + a.ln_eps);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int f = f0 + 16 * q + 4 * g;
      const f32x4 gm = *reinterpret_cast<const f32x4*>(a.ln_g + f);
      f32x4 y = (v[q] * rstd) * gm;
      if (a.ln_b) y += *reinterpret_cast<const f32x4*>(a.ln_b + f);
      v[q] = y;
    }
  }
  if (blockIdx.y == 0 && row_ok) {
#pragma unroll
    for (int q = 0; q < 2; ++q) *reinterpret_cast<f32x4*>(a.T + (long long)row * N + f0 + 16 * q + 4 * g) = v[q];
  }

  // ---- hand-over: the rows of t (+ add) become stage B's operand tile(s): small_chain_kernel's, once per tile
  if (need_add) {
#pragma unroll
    for (int q = 0; q < 2; ++q) w[q] = v[q] + w[q];
    atomicMax(&rmax[1][j], l3_absmax8(w[0], w[1]));
  }
  if (need_plain) atomicMax(&rmax[2][j], l3_absmax8(v[0], v[1]));
  __syncthreads();
  auto hand_over = [&](const f32x4 (&r)[2], unsigned maxbits, u32x4* tile) __attribute__((always_inline)) {
    float sc, inv;
    l3_scale(maxbits, 14, sc, inv);
    _Float16* dst = reinterpret_cast<_Float16*>(tile);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      typedef _Float16 h4 __attribute__((ext_vector_type(4)));
      h4 hh, mm;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xsv = r[q][e] * sc;
        hh[e] = (_Float16)xsv;
        mm[e] = (_Float16)(xsv - (float)hh[e]);
      }
      const int unit = wave * 64 + (2 * q + (g >> 1)) * 16 + j;             // k-step = this wave's 32 features
      *reinterpret_cast<h4*>(dst + (size_t)unit * 8 + 4 * (g & 1)) = hh;
      *reinterpret_cast<h4*>(dst + (size_t)(KS * 64 + unit) * 8 + 4 * (g & 1)) = mm;
    }
  };
  if (need_add) hand_over(w, rmax[1][j], xs[1]);
  if (need_plain) hand_over(v, rmax[2][j], xs[0]);
  __syncthreads();

  // ---- stage B
  float sc_, sx_inv;
  l3_scale(rmax[my_add ? 1 : 2][j], 14, sc_, sx_inv);
  const u32x4* xt = xs[my_add ? 1 : 0] + lane;
  f32x4 acc[2][1];
  acc[0][0] = acc[1][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < KS; kb += SL_AHEAD) {
#pragma unroll
    for (int u = 0; u < SL_AHEAD; ++u) {
      const int ks = kb + u;
      const f16x8 bh[1] = {__builtin_bit_cast(f16x8, xt[ks * 64])}, bm[1] = {__builtin_bit_cast(f16x8, xt[KS * 64 + ks * 64])};
      l3_mfma3_pair<1>(afr[u], bh, bm, acc[0], acc[1]);
      __builtin_amdgcn_sched_barrier(0);
      if (ks + SL_AHEAD < KS) load_a(wlb, a.Nwb, ks + SL_AHEAD, afr[u]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    f32x4 t = (acc[q][0] * sx_inv) * eb_wi[q] + eb_bi[q];
    if (a.relu) t = __builtin_elementwise_maximum(t, (f32x4){0.f, 0.f, 0.f, 0.f});   // NaN-propagating, as torch.relu
    t += (f32x4){0.f, 0.f, 0.f, 0.f};                            // (small_linear_kernel's `+ residual` without one: -0 -> +0)
    if (row_ok) *reinterpret_cast<f32x4*>(a.Y + (long long)row * a.Nb + fb0 + 16 * q + 4 * g) = t;
  }
}

// returns UNIVS_OK, or UNIVS_ERR_NOT_IMPLEMENTED when the shape is not covered
int small_seam_f32(const float* x, const void* wpa, const float* winv_a, const float* bias_a, const float* residual, const float* ln_g,
                   const float* ln_b, float ln_eps, float* t, const float* add, const void* wpb, const float* winv_b, const float* bias_b,
                   int n_wb, int f_off, float* y, long long M, int Ka, int Na, int Nb, int relu, int add_features, hipStream_t st) {
  if (M <= 0 || Nb <= 0) return UNIVS_OK;
  auto mis = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
  if (Ka != SL_KMAX || Na != 32 * SL_WAVES || Nb % (32 * SL_WAVES) != 0 || n_wb % 4 != 0 || f_off % 4 != 0 || f_off < 0 || f_off + Nb > n_wb ||
      M > 16LL * 65535 || Nb / (32 * SL_WAVES) > 65535 || add_features < 0 || add_features % 32 != 0 || mis(x) || mis(wpa) || mis(winv_a) ||
      mis(bias_a) || mis(residual) || mis(ln_g) || mis(ln_b) || mis(t) || mis(add) || mis(wpb) || mis(winv_b) || mis(bias_b) || mis(y) ||
      M * (long long)std::max(Nb, Ka) * 4 >= 0x7FFFFFFFLL)
    return UNIVS_ERR_NOT_IMPLEMENTED;
  SlSeamArgs a{};
  a.X = x; a.Wa = reinterpret_cast<const u32x4*>(wpa); a.winv_a = winv_a; a.bias_a = bias_a; a.Res = residual; a.ln_g = ln_g; a.ln_b = ln_b;
  a.ln_eps = ln_eps; a.T = t; a.Add = add; a.Wb = reinterpret_cast<const u32x4*>(wpb); a.winv_b = winv_b; a.bias_b = bias_b; a.Y = y;
  a.M = (int)M; a.Nb = Nb; a.Nwb = n_wb; a.f_off = f_off; a.relu = relu ? 1 : 0; a.add_features = add_features;
  hipLaunchKernelGGL(small_seam_kernel, dim3((unsigned)((M + 15) / 16), (unsigned)(Nb / (32 * SL_WAVES))), dim3(64 * SL_WAVES), 0, st, a);
  return check_launch("small_seam_f32");
}

}  // namespace univs
