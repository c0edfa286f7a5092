// Causal self-attention over PACKED sequences of unequal length (the CLIP text tower on its real tokens only), gfx950, fp32.
//
// qkv [Ntok, 3 E] is the packed in-projection of every sequence's kept tokens; sequence s owns rows start[s] .. start[s + 1].  Row i of a
// sequence gets softmax(scale q_i . k_{j <= i}) v_{j <= i} per head: nn.MultiheadAttention's core under the tower's upper-triangular
// mask.  A templated class name holds 4 to 13 tokens of the 77 the dense tower computes, so the [N, h, 77, 77] scores never exist here.
//
// One wave (a 64-thread workgroup) per (sequence, head).  K and V of the head lie in LDS, [Lmax][D + 1] floats each: lane j reads key
// j's row in the score step, and the odd row stride puts the 32 lanes of a ds_read_b32 group on 32 different banks (stride D would put
// them all on one).  Lane j holds the scores of keys j and j + 64 (lengths up to 128), the maximum and the sum are wave reductions, q_i
// is one coalesced load whose channels reach the lanes as scalar broadcasts (readlane with a constant lane).  In the P V step lane c
// owns channel c; where D < 64 the 64 / D lane groups take the keys in turn and meet with D-strided shuffles.  The probabilities pass
// from "lane = key" to "every lane reads key j" through 128 floats of LDS (one address per read: a broadcast).
//
// Untrusted table: the length is clamped to [0, Lmax] and the first row to [0, Ntok - length], so that no entry of `start` moves a
// read or a store outside the two tensors or the LDS image.  Arithmetic: fmaf chains, expf(score - rowmax), one division per row.
#include "launchers.h"

namespace univs {

constexpr int TEXT_ATTN_MAX_LEN = 128;

__device__ __forceinline__ float ta_wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float ta_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <int D>
__global__ __launch_bounds__(64) void text_attention_kernel(const float* __restrict__ qkv, const int* __restrict__ start, long long Ntok, int E,
                                                            int heads, int Lmax, float scale, float* __restrict__ out) {
  constexpr int STR = D + 1;                                       // odd: key-per-lane reads are conflict-free
  constexpr int G = 64 / D;                                        // lane groups of the P V step
  extern __shared__ float text_attn_lds[];
  float* Ks = text_attn_lds;                                       // [Lmax][STR]
  float* Vs = Ks + (size_t)Lmax * STR;                             // [Lmax][STR]
  float* Ps = Vs + (size_t)Lmax * STR;                             // [128]
  const int lane = threadIdx.x;
  const int s = blockIdx.x / heads, h = blockIdx.x - s * heads;
  const long long a = start[s], b = start[s + 1];
  const int n = (int)min(max(b - a, 0LL), (long long)min(Lmax, TEXT_ATTN_MAX_LEN));
  const long long row0 = min(max(a, 0LL), Ntok - n);               // (< 0: more keys than the tensor has rows -- nothing is done)
  if (n <= 0 || row0 < 0) return;
  const size_t ld = (size_t)3 * E;
  const float* base = qkv + (size_t)row0 * ld + (size_t)h * D;
  for (int idx = lane; idx < n * D; idx += 64) {                   // K and V of the head: rows of D consecutive floats
    const int j = idx / D, c = idx - j * D;
    Ks[j * STR + c] = base[(size_t)j * ld + E + c];
    Vs[j * STR + c] = base[(size_t)j * ld + 2 * E + c];
  }
  __syncthreads();
  const bool two = n > 64;
  const float* k0 = Ks + min(lane, n - 1) * STR;                   // (lanes beyond the sequence read its last key; masked below)
  const float* k1 = Ks + min(lane + 64, n - 1) * STR;
  const int g = lane / D, c = lane - g * D;
  for (int i = 0; i < n; ++i) {
    const int qbits = __float_as_int(lane < D ? base[(size_t)i * ld + lane] * scale : 0.f);
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int cc = 0; cc < D; ++cc) {
      const float qc = __int_as_float(__builtin_amdgcn_readlane(qbits, cc));
      s0 = fmaf(qc, k0[cc], s0);
      if (two) s1 = fmaf(qc, k1[cc], s1);
    }
    const bool in0 = lane <= i, in1 = two && lane + 64 <= i;
    const float m = ta_wave_max(fmaxf(in0 ? s0 : -INFINITY, in1 ? s1 : -INFINITY));   // (key 0 is always attended: m is finite)
    const float p0 = in0 ? expf(s0 - m) : 0.f, p1 = in1 ? expf(s1 - m) : 0.f;
    const float inv = 1.f / ta_wave_sum(p0 + p1);
    Ps[lane] = p0;
    Ps[lane + 64] = p1;
    __syncthreads();
    float acc = 0.f;
    for (int j = g; j <= i; j += G) acc = fmaf(Ps[j], Vs[j * STR + c], acc);
#pragma unroll
    for (int off = D; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);
    if (lane < D) out[(size_t)(row0 + i) * E + (size_t)h * D + lane] = acc * inv;
    __syncthreads();                                               // Ps is rewritten by the next row
  }
}

constexpr size_t TEXT_ATTN_MAX_LDS = ((size_t)2 * TEXT_ATTN_MAX_LEN * (64 + 1) + 128) * sizeof(float);   // 67 072 B: Lmax = 128, D = 64

// false: the runtime refused the LDS size (reported through set_error); nothing was launched
template <int D>
static bool launch_text_attention(const float* qkv, const int* start, int S, long long Ntok, int E, int heads, int Lmax, float scale, float* out,
                                  hipStream_t st) {
  const size_t lds = ((size_t)2 * Lmax * (D + 1) + 128) * sizeof(float);
  if (lds > 64 * 1024) {
    // above the default limit of dynamic LDS the kernel is allowed the largest image any call needs, once per device (the attribute
    // belongs to the device's copy of the code; two threads that both find it unset both set it, to the same value)
    static bool asked[64] = {};
    static hipError_t answer[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int slot = dev & 63;
    if (!asked[slot]) {
      answer[slot] = hipFuncSetAttribute(reinterpret_cast<const void*>(&text_attention_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)TEXT_ATTN_MAX_LDS);
      asked[slot] = answer[slot] == hipSuccess;                      // (a refusal is asked again, and reported again, next time)
    }
    const hipError_t allowed = answer[slot];
    if (allowed != hipSuccess) {
      set_error("text_attention_f32: %zu bytes of LDS refused: %s", lds, hipGetErrorString(allowed));
      return false;
    }
  }
  hipLaunchKernelGGL(text_attention_kernel<D>, dim3((unsigned)((long long)S * heads)), dim3(64), lds, st, qkv, start, Ntok, E, heads, Lmax, scale,
                     out);
  return true;
}

int text_attention_f32(const float* qkv, const int* start, int S, long long Ntok, int E, int heads, int Lmax, float scale, float* out,
                       hipStream_t st) {
  const int D = E / heads;
  if ((D != 16 && D != 32 && D != 64) || Lmax > TEXT_ATTN_MAX_LEN || Ntok * 3 * E >= (1LL << 31) || (long long)S * heads >= (1LL << 31))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  const bool ok = D == 16   ? launch_text_attention<16>(qkv, start, S, Ntok, E, heads, Lmax, scale, out, st)
                  : D == 32 ? launch_text_attention<32>(qkv, start, S, Ntok, E, heads, Lmax, scale, out, st)
                            : launch_text_attention<64>(qkv, start, S, Ntok, E, heads, Lmax, scale, out, st);
  return ok ? check_launch("text_attention_f32") : UNIVS_ERR_LAUNCH;
}

}  // namespace univs
