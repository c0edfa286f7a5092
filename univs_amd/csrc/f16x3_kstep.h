// One k-step of the three-product fp16 GEMM (f16x3.h; linear_f16x3.hip has the arithmetic) on a W image in LDS, for the kernels whose
// waves hold 16 RB features x 32 rows: linear_f16x3.hip and linear_pair_f16x3.hip (W resident) and gemm_f16x3_stream.hip (W streamed).
// The arithmetic contract -- split, scale rule and its numbers, product order -- lives in f16x3.h; this header applies it to those kernels'
// k-step, once:
//   * the A-fragment pipeline: W parts from LDS in batches, read one batch ahead of the matrix instructions that use them;
//   * the running row scale (l3_scale_* of f16x3.h) of one ring stage of x: two rows per lane;
//   * the three products (l3_mfma3_block) of one batch.
// conv3x3_wide.hip uses the same k-step on a W image that f16x3_wstream.h streams in.
// What differs between the kernels stays in them: the order in which x is refilled, W fetched and committed and the next batch read.
#pragma once
#include "f16x3.h"

namespace univs {

// A fragments (W parts) come from LDS in NB batches of BSZ feature blocks, software-pipelined by hand: the reads of batch
// b + 1 are issued BEFORE the 6 BSZ MFMAs of batch b and waited for after them.  Left to the compiler, every ds_read_b128
// sat directly in front of its first use behind an `s_waitcnt lgkmcnt(0)` (ISA of the first version): ~100 clocks of
// exposed LDS latency per 3 MFMAs, and halving the MFMA work against the six-product kernel changed nothing.
template <int RB>
struct KStep {
  static constexpr int Rp = 16 * RB;                             // rows of the LDS image
  static constexpr int NB = RB > 6 ? 4 : 2;                      // even: the two buffers alternate across k-steps too
  static constexpr int BSZ = (RB + NB - 1) / NB;                 // 1 .. 3 blocks
  typedef u32x4 Batch[BSZ][2];                                   // [block of the batch][part h, m]
  // byte address of (k-step ks, k-group g, part h, row j) of an image [k-step][4 k-groups][2 parts][Rp] of 16-byte units:
  // lane(g, j) + ks * kstep; blocks are 256 B apart, the m part Rp * 16 B further
  static constexpr unsigned kstep = (unsigned)(8 * Rp * 16);
  static __device__ __forceinline__ unsigned lane(int g, int j) { return (unsigned)((g * 2 * Rp + j) * 16); }
};

// read_batch(d, base, integral_constant<B>): batch B of the k-step at lane address `base` into d.  The block (256 B) and part offsets of a
// read are IMMEDIATES of the instruction (batch index = a compile-time constant): one address register per k-step instead of two vector
// adds per read (16 of ~100 vector instructions per k-step at 128 features).
// A lambda, handed out by a function -- `auto read_batch = l3_batch_reader<RB>();` -- and not a function template itself: as a function the
// same text leaves the fragments' phi nodes in another order, and the kernels of three blocks per batch get other registers
template <int RB>
__device__ __forceinline__ auto l3_batch_reader() {
  return [](typename KStep<RB>::Batch& d, unsigned base, auto bc) __attribute__((always_inline)) {
    constexpr int b = decltype(bc)::value;
    constexpr int BSZ = KStep<RB>::BSZ, Rp = KStep<RB>::Rp;
    l3_static_for<0, BSZ>([&](auto qc) __attribute__((always_inline)) {
      constexpr int q = decltype(qc)::value;
      constexpr int rb = b * BSZ + q < RB ? b * BSZ + q : RB - 1;   // a short last batch re-reads the last block
      u32x4& dh = d[q][0];                                       // (operands of an asm statement do not capture: name them first)
      u32x4& dm = d[q][1];
      const unsigned aa = base;
      asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
                   : "=&v"(dh), "=&v"(dm)
                   : "v"(aa), "n"(rb * 256), "n"(rb * 256 + Rp * 16)
                   : "memory");
    });
  };
}

// all LDS traffic in flight is the batch about to be used; the operands tie the MFMAs that follow to this wait
template <int BSZ>
__device__ __forceinline__ void l3_wait_batch(u32x4 (&d)[BSZ][2]) {
  if constexpr (BSZ == 1)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(d[0][0]), "+v"(d[0][1]) : : "memory");
  else if constexpr (BSZ == 2)
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(d[0][0]), "+v"(d[0][1]), "+v"(d[1][0]), "+v"(d[1][1]) : : "memory");
  else
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(d[0][0]), "+v"(d[0][1]), "+v"(d[1][0]), "+v"(d[1][1]), "+v"(d[2][0]), "+v"(d[2][1]) : : "memory");
}

// Row scales of x WITHOUT a pass of their own: a running scale per row.  Before a k-step is split its row maximum (over
// the four lanes that hold the row's k-groups) is compared with the exponent the current scale was set for; a row whose
// new maximum would leave fp16's range gets a smaller power of two, and the accumulators of that row -- sums of
// products under the old scale -- are multiplied by the ratio (exact).  The scale is set for 2^12 (three binades of room
// for later k-steps), only ever shrinks, and typically changes once or twice per row.
// State, three arrays of the kernel: `eset` the exponent the scale of my two rows (column tiles) was set for, `sx` the scale, `sx_inv` its
// inverse.  The step is two halves with the wave-wide vote between them at the call site:
//     int enew[2];
//     if (__builtin_amdgcn_ballot_w64(l3_row_scale_need(raw, eset, enew)) != 0) l3_row_scale_lower(enew, acc, eset, sx, sx_inv);   // rare
// (as one function, or with the state in one struct, every kernel compiles into longer code: DESIGN.md, "One k-step core").
// A new row tile: the first k-step sets the scale.  `frozen`: linear_f16x3's timing switch LA_SCALE_FROZEN -- the scale stays at 1, and
// the kernel skips the lowering.
__device__ __forceinline__ void l3_row_scale_reset(int (&eset)[2], float (&sx)[2], float (&sx_inv)[2], bool frozen = false) {
  eset[0] = eset[1] = frozen ? L3_SCALE_SET : -1000;
  sx[0] = sx[1] = sx_inv[0] = sx_inv[1] = 1.0f;
}

// one ring stage `raw` ([column tile][16-byte half]: 8 consecutive k of my two rows): the exponents of its row maxima, and whether one
// of my rows would leave the range its scale was set for
__device__ __forceinline__ bool l3_row_scale_need(const f32x4 (&raw)[2][2], const int (&eset)[2], int (&enew)[2]) {
  bool need = false;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const unsigned mk = l3_row_max(l3_absmax8(raw[c][0], raw[c][1]));
    enew[c] = l3_scale_exp(mk);
    need = need || l3_scale_stale(enew[c], eset[c]);
  }
  return need;
}

// ... and the smaller scale of such rows, with the exact rescaling of their accumulators (gemm_f16x3_stream.hip holds this text in
// place: a change here is a change there)
template <int RB>
__device__ __forceinline__ void l3_row_scale_lower(const int (&enew)[2], f32x4 (&acc)[RB][2], int (&eset)[2], float (&sx)[2],
                                                   float (&sx_inv)[2]) {
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int en = l3_scale_stale(enew[c], eset[c]) ? enew[c] : eset[c];
    const float ratio = l3_scale_ratio(eset[c], en);
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[rb][c] *= ratio;
    eset[c] = en;
    sx[c] = l3_scale_of(en);
    sx_inv[c] = l3_scale_inv_of(en);
  }
}

// the three products of batch B on the split stage (bh, bm) of x: six MFMAs per feature block, in f16x3.h's order
template <int RB, int B>
__device__ __forceinline__ void l3_mfma_batch(const typename KStep<RB>::Batch& a, const f16x8 (&bh)[2], const f16x8 (&bm)[2],
                                              f32x4 (&acc)[RB][2]) {
  constexpr int BSZ = KStep<RB>::BSZ;
#pragma unroll
  for (int q = 0; q < BSZ; ++q) {
    const int rb = B * BSZ + q;
    if (rb < RB) l3_mfma3_block<2>(__builtin_bit_cast(f16x8, a[q][0]), __builtin_bit_cast(f16x8, a[q][1]), bh, bm, acc[rb]);
  }
}

}  // namespace univs
