// The merge of the key segments' partial results of the attention core (cross_attn.hip: xattn_partial writes, per (query, batch entry,
// head) and segment p, XA_PART floats: O_p[32] unnormalised, the running maximum m_p in log2 units, the sum l_p):
//   out[c] = sum_p O_p[c] 2^(m_p - M) / sum_p l_p 2^(m_p - M),  M = max_p m_p
// ONE statement of it, used by xattn_merge (a thread per channel) and by the out-projection that merges while it stages its operand
// (small_linear.hip: a thread per eight channels): the same operations in the same order, so the same bits by construction.
#pragma once
#include <hip/hip_runtime.h>

namespace univs {

constexpr int XA_PART = 34;

// `base`: the first segment's record; `pstride`: floats between the records of two segments; channels c0 ... c0 + NC - 1
template <int NC>
__device__ __forceinline__ void xa_merge_partials(const float* __restrict__ base, long long pstride, int nseg, int c0, float (&out)[NC]) {
  float M = -INFINITY;
#pragma unroll 8                                                 // (independent loads in flight: pure latency)
  for (int p = 0; p < nseg; ++p) M = fmaxf(M, base[p * pstride + 32]);
  float acc[NC], l = 0.f;
#pragma unroll
  for (int e = 0; e < NC; ++e) acc[e] = 0.f;
#pragma unroll(NC == 1 ? 8 : 4)
  for (int p = 0; p < nseg; ++p) {
    const float f = __builtin_amdgcn_exp2f(base[p * pstride + 32] - M);
#pragma unroll
    for (int e = 0; e < NC; ++e) acc[e] = fmaf(base[p * pstride + c0 + e], f, acc[e]);
    l = fmaf(base[p * pstride + 33], f, l);
  }
#pragma unroll
  for (int e = 0; e < NC; ++e) out[e] = acc[e] / l;
}

}  // namespace univs
