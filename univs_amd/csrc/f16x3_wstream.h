// The weight stream of the three-product kernels whose OPERAND is resident in registers (mlp_f16x3.hip, linear_pair_xres.hip) or walked
// once (conv3x3_wide.hip): the pre-split image of W goes global -> LDS by DMA into a ring of images, and a wave reads its A fragments --
// two feature blocks x two parts per batch -- from the current image TWO batches ahead of the matrix instructions, into a ring of three,
// with counted waits.  The pieces every such kernel needs, once:
//   * l3_glds16: one wave's 1-KB piece of the stream;
//   * l3_read4: the four ds_read_b128 of a batch;
//   * l3_wait_lgkm<N>: the counted wait in front of a batch's products.
// What differs between the kernels stays in them and is documented at their loops: ring depth, which slot requests which piece, the
// counted vmcnt in front of a barrier, where the barriers sit.  The arithmetic (product order, scale rule) is f16x3.h's.
#pragma once
#include "f16x3.h"

namespace univs {

// One wave's 1-KB piece: lane l's 16 bytes at `base` + `voff` -> LDS byte address `lds_dst` + 16 l.  `base` and `lds_dst` are wave-uniform;
// the lane's part of the address is a 32-bit offset (no 64-bit vector arithmetic in the stream).  The instruction takes its LDS destination
// from M0, which the compiler does not preserve around asm statements: it is saved, written and restored in the statement that uses it (the
// s_nop covers the wait state between a write of M0 and the DMA).  readfirstlane: an "s" operand that the compiler happens to hold in a
// vector register would be passed as one.
// The request is NOT in hipcc's vmcnt bookkeeping: the kernel waits for it with a counted `s_waitcnt vmcnt` of its own.
__device__ __forceinline__ void l3_glds16(const u32x4* base, unsigned voff, unsigned lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(base), "s"(dst) : "memory");
}
// ... with a 64-bit address per lane (the MLP kernels: a piece there is not contiguous in the image of W1)
__device__ __forceinline__ void l3_glds16(const u32x4* gsrc, unsigned lds_dst) {
  unsigned keep;
  const unsigned dst = __builtin_amdgcn_readfirstlane(lds_dst);
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(gsrc), "s"(dst) : "memory");
}

// A batch of fragments d[block][part h, m] from the image at lane address `addr`, the four byte offsets as IMMEDIATES of the reads (one
// address register per image instead of vector adds per read) ...
template <int O00, int O01, int O10, int O11>
__device__ __forceinline__ void l3_read4(u32x4 (&d)[2][2], unsigned addr) {
  asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\tds_read_b128 %3, %4 offset:%8"
               : "=&v"(d[0][0]), "=&v"(d[0][1]), "=&v"(d[1][0]), "=&v"(d[1][1])
               : "v"(addr), "n"(O00), "n"(O01), "n"(O10), "n"(O11)
               : "memory");
}
// ... or with the part stride in a register (the MLP kernels: it differs between their two products); blocks are 256 B apart
__device__ __forceinline__ void l3_read4(u32x4 (&d)[2][2], unsigned addr, unsigned pstride) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const unsigned ah = addr + (unsigned)(q * 256);
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3" : "=&v"(d[q][0]), "=&v"(d[q][1]) : "v"(ah), "v"(ah + pstride) : "memory");
  }
}

// At most N LDS operations of this wave are still in flight: N = those issued after the batch's reads (LDS operations complete in order,
// and the loops hold no scalar memory operation, so the count is exact).  The operands tie the matrix instructions that follow to the wait.
template <int N>
__device__ __forceinline__ void l3_wait_lgkm(u32x4 (&d)[2][2]) {
  static_assert(0 <= N && N <= 15, "lgkmcnt is a 4-bit counter");
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(d[0][0]), "+v"(d[0][1]), "+v"(d[1][0]), "+v"(d[1][1]) : "n"(N) : "memory");
}

}  // namespace univs
