// The arithmetic contract of the three-product kernels, once: the fp16 two-part split, the row-scale rules and their numbers, the product
// order (l3_mfma3_block / l3_mfma3_pair), GELU and the instrumentation macros.  Included by f16x3_kstep.h (the k-step of the W-in-LDS pass
// kernels) and f16x3_wstream.h (the LDS-DMA weight stream of the operand-resident kernels), gemm_f16x3_tile.hip, small_linear.hip and the
// attention cores (cross_attn.hip, window_attn_f16.hip: the split only).
#pragma once
#include "common.h"

#include <type_traits>

namespace univs {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the numbers of the row-scale rules: the running scale's set point, the margin before it is lowered, the clamp of a row maximum's
// exponent and of the exponent of an accumulator ratio
constexpr int L3_SCALE_SET = 12, L3_SCALE_MARGIN = 2, L3_EXP_MIN = -100, L3_EXP_MAX = 128, L3_RATIO_MIN = -126;

// power of two that brings a row whose largest magnitude has the bit pattern `maxbits` into [2^t, 2^(t+1)), and its inverse.
// Zero rows and rows below 2^-100 keep a finite scale (2^(t+100)); an infinite maximum gives 2^(t-128).
__device__ __forceinline__ void l3_scale(unsigned maxbits, int t, float& s, float& inv) {
  int e = (int)((maxbits >> 23) & 255u) - 127;            // 2^e <= max < 2^(e+1)
  e = max(L3_EXP_MIN, min(e, L3_EXP_MAX));
  s = __builtin_bit_cast(float, (unsigned)(127 + t - e) << 23);
  inv = __builtin_bit_cast(float, (unsigned)(127 - t + e) << 23);
}

// The RUNNING row scale's rule (f16x3_kstep.h has the state and the two-row step; gemm_f16x3_tile.hip, linear_pair_xres.hip and
// mlp_f16x3.hip keep their own state): a row's scale is set for exponent `eset` -- values up to 2^(eset + 1) land below
// 2^(L3_SCALE_SET + 1) --, is stale once a k-step's maximum has an exponent more than L3_SCALE_MARGIN above it, and is then set anew for
// that exponent, the row's accumulators multiplied by the exact ratio 2^(old - new) <= 1.  The numbers exist here only.
__device__ __forceinline__ int l3_scale_exp(unsigned maxbits) {              // 2^e <= max < 2^(e+1), clamped
  return max(L3_EXP_MIN, min((int)((maxbits >> 23) & 255u) - 127, L3_EXP_MAX));
}
__device__ __forceinline__ bool l3_scale_stale(int enew, int eset) { return enew > eset + L3_SCALE_MARGIN; }
__device__ __forceinline__ unsigned l3_scale_ratio_exp(int eold, int enew) {  // biased exponent of the ratio
  return (unsigned)(127 + max(eold - enew, L3_RATIO_MIN));
}
__device__ __forceinline__ float l3_scale_ratio(int eold, int enew) { return __builtin_bit_cast(float, l3_scale_ratio_exp(eold, enew) << 23); }
__device__ __forceinline__ float l3_scale_of(int e) { return __builtin_bit_cast(float, (unsigned)(127 + L3_SCALE_SET - e) << 23); }
__device__ __forceinline__ float l3_scale_inv_of(int e) { return __builtin_bit_cast(float, (unsigned)(127 - L3_SCALE_SET + e) << 23); }

// Timing experiments only (instrumented builds, `python -m univs_amd.build --ablate nosplit|nomfma|nosplit_nomfma`; results WRONG):
//   UNIVS_ABLATE_NOSPLIT -- the x operand is taken as if it arrived pre-split (its 32 bytes per lane reinterpreted as the two fp16x8
//   parts, no row maximum, no conversions): what a consumer of producer-side (hi, lo) activations would execute;
//   UNIVS_ABLATE_NOMFMA  -- the matrix instructions are dropped (operands kept alive).
#ifdef UNIVS_ABLATE_NOMFMA
__device__ __forceinline__ f32x4 l3_fake_mfma(f16x8 a, f16x8 b, f32x4 c) {
  asm volatile("" : "+v"(c) : "v"(a), "v"(b));
  return c;
}
#define __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, x, y, z) l3_fake_mfma(a, b, c)
#endif

// THE PRODUCT ORDER of the family, and the only place its matrix instruction is spelled out (mlp_f16x3_ps issues the same order through
// its ML_PS_MMA): per k-step of 32 the three products smallest terms first -- m h', h m', h h' -- where (h, m) are the parts of W and
// (h', m') those of the operand, each product over all CT column tiles before the next.
// One feature block (parts ah, am) on CT column tiles: acc[ct] += W_block x_ct^T
template <int CT>
__device__ __forceinline__ void l3_mfma3_block(f16x8 ah, f16x8 am, const f16x8 (&bh)[CT], const f16x8 (&bm)[CT], f32x4 (&acc)[CT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(am, bh[ct], acc[ct], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bm[ct], acc[ct], 0, 0, 0);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[ct], acc[ct], 0, 0, 0);
}
// Two feature blocks (fragments fr[block][part h, m]) alternating, so that dependent accumulators are two issues apart
template <int CT>
__device__ __forceinline__ void l3_mfma3_pair(const u32x4 (&fr)[2][2], const f16x8 (&bh)[CT], const f16x8 (&bm)[CT], f32x4 (&c0)[CT],
                                              f32x4 (&c1)[CT]) {
  const f16x8 ah0 = __builtin_bit_cast(f16x8, fr[0][0]), am0 = __builtin_bit_cast(f16x8, fr[0][1]);
  const f16x8 ah1 = __builtin_bit_cast(f16x8, fr[1][0]), am1 = __builtin_bit_cast(f16x8, fr[1][1]);
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    c0[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(am0, bh[ct], c0[ct], 0, 0, 0);
    c1[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(am1, bh[ct], c1[ct], 0, 0, 0);
  }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    c0[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah0, bm[ct], c0[ct], 0, 0, 0);
    c1[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah1, bm[ct], c1[ct], 0, 0, 0);
  }
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    c0[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah0, bh[ct], c0[ct], 0, 0, 0);
    c1[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah1, bh[ct], c1[ct], 0, 0, 0);
  }
}

// UNIVS_TRACE_GEMM (instrumented build `--ablate trace`): s_memtime stamps of a few (workgroup, wave) pairs at the phase boundaries of
// linear_f16x3 / gemm_f16x3_stream, read back through univs_debug_gemm_trace_{linear,stream} (tools/gemm_trace.py).
#ifdef UNIVS_TRACE_GEMM
#define UNIVS_GT_SLOTS 48
#define UNIVS_GT_STAMPS 64
#define UNIVS_GT_DECL(sym) static __device__ unsigned long long sym[UNIVS_GT_SLOTS * UNIVS_GT_STAMPS]
// slot: workgroups x = {0, mid, last} of passes y = {0, last}, all 8 waves; -1 elsewhere
#define UNIVS_GT_SLOT()                                                                                                     \
  ((((int)blockIdx.x == 0 || (int)blockIdx.x == (int)gridDim.x / 2 || (int)blockIdx.x == (int)gridDim.x - 1) &&                \
    ((int)blockIdx.y == 0 || (int)blockIdx.y == (int)gridDim.y - 1))                                                          \
       ? ((((int)blockIdx.x == 0 ? 0 : (int)blockIdx.x == (int)gridDim.x - 1 ? 2 : 1) * 2 + ((int)blockIdx.y == 0 ? 0 : 1)) * 8 + \
          (int)(threadIdx.x >> 6))                                                                                            \
       : -1)
#define UNIVS_GT(sym, slot, i)                                                                                  \
  do {                                                                                                          \
    if ((slot) >= 0 && (threadIdx.x & 63) == 0 && (i) < UNIVS_GT_STAMPS) sym[(slot) * UNIVS_GT_STAMPS + (i)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#define UNIVS_GT_REAL(sym, slot, i)                                                                             \
  do {                                                                                                          \
    if ((slot) >= 0 && (threadIdx.x & 63) == 0) sym[(slot) * UNIVS_GT_STAMPS + (i)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define UNIVS_GT_VAL(sym, slot, i, v)                                                                           \
  do {                                                                                                          \
    if ((slot) >= 0 && (threadIdx.x & 63) == 0) sym[(slot) * UNIVS_GT_STAMPS + (i)] = (unsigned long long)(v);  \
  } while (0)
#else
#define UNIVS_GT_SLOT() (-1)
#define UNIVS_GT(sym, slot, i) do { } while (0)
#define UNIVS_GT_REAL(sym, slot, i) do { } while (0)
#define UNIVS_GT_VAL(sym, slot, i, v) do { } while (0)
#endif

// f(integral_constant<int, I>) for I = I0 .. N - 1: loops whose index has to be a compile-time constant (immediate offsets of asm
// statements; `#pragma unroll` is a hint and its index is not a constant expression)
template <int I, int N, class F>
__device__ __forceinline__ void l3_static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    l3_static_for<I + 1, N>(f);
  }
}

// 8 consecutive k of one row, scaled -> the two fp16x8 parts (round to nearest even)
__device__ __forceinline__ void l3_split8(f32x4 v0, f32x4 v1, float s, f16x8& h, f16x8& m) {
#ifdef UNIVS_ABLATE_NOSPLIT
  h = __builtin_bit_cast(f16x8, v0);
  m = __builtin_bit_cast(f16x8, v1);
  return;
#endif
#ifdef UNIVS_SPLIT_PLAIN   // (A / B: the plain expression, ~3.4 vector instructions per value as hipcc compiles it; same values)
  {
    const float xp[8] = {v0.x * s, v0.y * s, v0.z * s, v0.w * s, v1.x * s, v1.y * s, v1.z * s, v1.w * s};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const _Float16 hh = (_Float16)xp[e];
      h[e] = hh;
      m[e] = (_Float16)(xp[e] - (float)hh);                  // exact difference, then rounded
    }
    return;
  }
#endif
  // Two instructions per value, written into the packed halves directly: h = fp16(v s) and m = fp16(v s - h) as mixed-precision FMAs
  // (v_fma_mix{lo,hi}_f16: fp32 sources v and s, the third source 0 or -h read as fp16 from the half just written; one rounding each).
  // The same values as the mul / cvt / cvt-back / sub / cvt chain hipcc makes of the plain expression -- s is a power of two, so v s
  // is exact, and v s - fp16(v s) is exact in fp32 -- at 2 instead of ~3.4 vector instructions per value: the split is a fifth of the
  // vector work of every three-product kernel, and vector work does not overlap the matrix pipe (profiles/r05_gemm_negative_results_v2.txt).
  const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
  u32x4 hu, mu;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned hp, mp;
    asm("v_fma_mixlo_f16 %0, %2, %4, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %3, %4, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %1, %2, %4, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %3, %4, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(hp), "=&v"(mp)
        : "v"(x[2 * p]), "v"(x[2 * p + 1]), "v"(s));
    hu[p] = hp;
    mu[p] = mp;
  }
  h = __builtin_bit_cast(f16x8, hu);
  m = __builtin_bit_cast(f16x8, mu);
}

// The same two-instruction split without a scale, for the attention cores (cross_attn.hip, window_attn_f16.hip), whose operands are
// range-scaled beforehand where they need it: two values -> one packed pair of first parts h = fp16(x) and one of second parts
// m = fp16(x - h).  The same bits as `h = (_Float16)x; m = (_Float16)(x - (float)h)`: fp16(x 1 + 0) is the one rounding of the
// conversion, and x - h is exact in fp32 (h holds x's leading 11 bits), so fp16(fma(x, 1, -h)) rounds the same number once.
__device__ __forceinline__ void l3_split2(float x0, float x1, unsigned& hp, unsigned& mp) {
  asm("v_fma_mixlo_f16 %0, %2, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixhi_f16 %0, %3, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
      "v_fma_mixlo_f16 %1, %2, 1.0, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %1, %3, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "=&v"(hp), "=&v"(mp)
      : "v"(x0), "v"(x1));
}
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
// PADDED: for values that come straight from a transcendental instruction (v_exp_f32: no vector instruction may read its result in
// the very next slot) and parts that go straight into a matrix instruction (two wait states after the vector write).  hipcc keeps such
// distances between its own instructions only, not around an asm statement, so the split is ONE statement that opens and closes with them.
template <bool PADDED = false>
__device__ __forceinline__ void l3_split8(const float (&x)[8], f16x8& h, f16x8& m) {
  u32x4 hu, mu;
  if constexpr (PADDED) {
    unsigned h0, h1, h2, h3, m0, m1, m2, m3;
    asm("s_nop 0\n\t"
        "v_fma_mixlo_f16 %0, %8, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %9, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %4, %8, 1.0, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %4, %9, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %1, %10, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %11, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %5, %10, 1.0, -%1 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %5, %11, 1.0, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %2, %12, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %2, %13, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %6, %12, 1.0, -%2 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %6, %13, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %3, %14, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %3, %15, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %7, %14, 1.0, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %7, %15, 1.0, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(h0), "=&v"(h1), "=&v"(h2), "=&v"(h3), "=&v"(m0), "=&v"(m1), "=&v"(m2), "=&v"(m3)
        : "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]));
    hu = (u32x4){h0, h1, h2, h3};
    mu = (u32x4){m0, m1, m2, m3};
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      unsigned hp, mp;
      l3_split2(x[2 * p], x[2 * p + 1], hp, mp);
      hu[p] = hp;
      mu[p] = mp;
    }
  }
  h = __builtin_bit_cast(f16x8, hu);
  m = __builtin_bit_cast(f16x8, mu);
}
template <bool PADDED = false>
__device__ __forceinline__ void l3_split4(float x0, float x1, float x2, float x3, f16x4& h, f16x4& m) {
  u32x2 hu, mu;
  unsigned h0, h1, m0, m1;
  if constexpr (PADDED) {
    asm("s_nop 0\n\t"
        "v_fma_mixlo_f16 %0, %4, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %0, %5, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %2, %4, 1.0, -%0 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %2, %5, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixlo_f16 %1, %6, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixhi_f16 %1, %7, 1.0, 0 op_sel_hi:[0,0,0]\n\t"
        "v_fma_mixlo_f16 %3, %6, 1.0, -%1 op_sel:[0,0,0] op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %3, %7, 1.0, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
        "s_nop 1"
        : "=&v"(h0), "=&v"(h1), "=&v"(m0), "=&v"(m1)
        : "v"(x0), "v"(x1), "v"(x2), "v"(x3));
  } else {
    l3_split2(x0, x1, h0, m0);
    l3_split2(x2, x3, h1, m1);
  }
  hu = (u32x2){h0, h1};
  mu = (u32x2){m0, m1};
  h = __builtin_bit_cast(f16x4, hu);
  m = __builtin_bit_cast(f16x4, mu);
}

__device__ __forceinline__ unsigned l3_absmax8(f32x4 v0, f32x4 v1) {
#ifdef UNIVS_ABLATE_NOSPLIT
  return 0x3f800000u;
#endif
#ifdef UNIVS_SPLIT_PLAIN
  {
    const float a = fmaxf(fmaxf(fabsf(v0.x), fabsf(v0.y)), fmaxf(fabsf(v0.z), fabsf(v0.w)));
    const float b = fmaxf(fmaxf(fabsf(v1.x), fabsf(v1.y)), fmaxf(fabsf(v1.z), fabsf(v1.w)));
    return __builtin_bit_cast(unsigned, fmaxf(a, b));
  }
#endif
  // max |.| of eight values in four instructions (v_max3_f32 with |.| source modifiers)
  float t1, t2, r;
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(t1) : "v"(v0.x), "v"(v0.y), "v"(v0.z));
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(t2) : "v"(v0.w), "v"(v1.x), "v"(v1.y));
  asm("v_max3_f32 %0, |%1|, |%2|, %3" : "=v"(r) : "v"(v1.z), "v"(v1.w), "v"(t1));
  return __builtin_bit_cast(unsigned, fmaxf(r, t2));       // non-negative floats order like their bit patterns
}

// nn.GELU() (approximate = 'none'): x * 0.5 * (1 + erf(x / sqrt 2)) with erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7;
// in fp32 the GELU differs from the exact value by <= 4.7e-7 absolute on [-12, 12], ATen's own fp32 GELU by 1.2e-6): one
// reciprocal, one exp2 and eight multiply-adds, branch-free -- the library's erff (three ranges under lane divergence) was
// a third of the fc1 + GELU kernels' time.
__device__ __forceinline__ float l3_gelu(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float p = fmaf(t, 1.061405429f, -1.453152027f);
  p = fmaf(t, p, 1.421413741f);
  p = fmaf(t, p, -0.284496736f);
  p = fmaf(t, p, 0.254829592f);
  p *= t;
  const float e = __builtin_amdgcn_exp2f(-(z * z) * 1.4426950408889634f);
  const float erf_abs = fmaf(-p, e, 1.0f);
  const float erf = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, erf_abs) | (__builtin_bit_cast(unsigned, x) & 0x80000000u));
  return 0.5f * x * (1.0f + erf);
}

// maximum over the four lanes (k-groups, lane >> 4) that hold one row of the B operand
__device__ __forceinline__ unsigned l3_row_max(unsigned v) {
#ifdef UNIVS_ABLATE_NOSPLIT
  return v;
#endif
  const auto s1 = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  const unsigned r1 = max(s1[0], s1[1]);
  const auto s2 = __builtin_amdgcn_permlane16_swap(r1, r1, false, false);
  return max(s2[0], s2[1]);
}

}  // namespace univs
