// The exact-f32 contraction of the mask decode, shared by its two users: csrc/mask_decode.hip (logits and attention-mask bytes are
// STORED) and csrc/semantic_decode.hip (logits are only COUNTED against two thresholds).  One pair of kernel templates and one launcher,
// so a logit has one arithmetic wherever it is formed: v_mfma_f32_32x32x2_f32 is an exact k-ordered fp32 fmaf chain, and a count taken
// here can never disagree with the same logit stored by ops.mask_decode under the exact-f32 setting.
//
// An epilogue is either a STORING one -- `ep(t, q, col, N, v)` per valid element, as before -- or a ROW-COUNTING one, recognised by its
// members `count`, `flush` and `t_step`:
//   * the kernel's frame is blockIdx.z * ep.t_step (the storing epilogues walk every frame);
//   * 2 * QP ints of LDS behind the A tile are zeroed before the first barrier;
//   * `ep.count(tab, row, valid, v)` is called by ALL 64 lanes for each accumulator register (row = the lane's row inside the block
//     tile; valid = the column is inside N and the row inside Q -- clamped columns and padded rows hold copies or zeros);
//   * `ep.flush(tab, q0, QP, tid)` runs once per workgroup after a barrier behind the last tile.
// The storing instantiations compile to what they were before the hooks: every hook sits under `if constexpr`.
#pragma once
#include "common.h"
#include "config.h"

#include <type_traits>

namespace univs {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MD_THREADS = 512;   // 8 waves = 2 per SIMD: one wave's HBM latency hides under the other's MFMAs
constexpr int MD_WAVE_N = 32;     // columns per wave per tile
constexpr int MD_BLOCK_N = 256;   // 8 waves x 32 columns

template <typename E, typename = void>
struct CountsRows : std::false_type {};
template <typename E>
struct CountsRows<E, std::void_t<decltype(&E::count), decltype(&E::flush), decltype(E::t_step)>> : std::true_type {};

// MI = number of 32-row blocks of A handled by each wave (rows per block-tile = 32*MI).
// B fragments are fetched with raw buffer loads: the per-lane byte offset (column, k parity) is
// computed once, the k-row offset travels in an SGPR, out-of-range columns are clamped (their results
// are never stored) -- no per-load VALU address arithmetic and no divergent control flow, so the 16
// loads of a chunk are in flight together and the NEXT chunk is fetched while the current one feeds
// the MFMAs (register double buffer).
template <int MI, typename Epilogue>
__global__ __launch_bounds__(MD_THREADS, 1) void skinny_gemm_f32(const float* __restrict__ A,  // [T,Q,K]
                                                                  const float* __restrict__ B,  // [T,K,N]
                                                                  int Q, int K, long long N,
                                                                  int tiles_per_block, Epilogue ep) {
  extern __shared__ __attribute__((aligned(16))) float At[];  // [K][LDP]
  constexpr int QP = 32 * MI;
  constexpr int LDP = QP + 1;
  constexpr int UNR = 16;  // k-steps (of 2) per chunk
  constexpr bool RC = CountsRows<Epilogue>::value;
  int frame = blockIdx.z;
  if constexpr (RC) frame *= ep.t_step;
  const int t = frame;
  const int q0 = blockIdx.y * QP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* rowtab = nullptr;   // [QP][2], row-counting epilogues only
  if constexpr (RC) {
    rowtab = reinterpret_cast<int*>(At + K * LDP);
    for (int i = tid; i < 2 * QP; i += MD_THREADS) rowtab[i] = 0;
  }

  // ---- stage A^T (rows q0..q0+QP) into LDS; coalesced along k, bank = (k + q) % 32 on the write
  const float* At_src = A + ((long long)t * Q) * K;
  for (int idx = tid; idx < QP * K; idx += MD_THREADS) {
    const int k = idx % K, q = idx / K;
    At[k * LDP + q] = (q0 + q < Q) ? At_src[(long long)(q0 + q) * K + k] : 0.f;
  }
  __syncthreads();

  const int khalf = lane >> 5;   // which of the two k's of an MFMA this lane feeds
  const int l31 = lane & 31;
  const int Ni = (int)N;
  // buffer resource over this frame's B matrix (K*N floats); wave-uniform by construction
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(B + (long long)t * K * N), 0, (int)((long long)K * N * 4), 0x00020000);
  const int Kc = (K + 2 * UNR - 1) / (2 * UNR);  // chunks; rows >= K read as 0 (buffer bounds check)

  for (int tile = 0; tile < tiles_per_block; ++tile) {
    const long long col0 = ((long long)blockIdx.x * tiles_per_block + tile) * MD_BLOCK_N + wave * MD_WAVE_N;
    if (col0 >= N) break;                    // wave-uniform
    const int col = (int)col0 + l31;
    const bool cv = col < Ni;
    const int voff = (min(col, Ni - 1) + khalf * Ni) * 4;  // bytes

    f32x16 acc[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

    float bcur[UNR], bnext[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      bcur[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (2 * u) * Ni * 4, 0));

    for (int c = 0; c < Kc; ++c) {
      const int k0 = c * 2 * UNR;
      if (c + 1 < Kc) {
#pragma unroll
        for (int u = 0; u < UNR; ++u)
          bnext[u] = __builtin_bit_cast(
              float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (k0 + 2 * UNR + 2 * u) * Ni * 4, 0));
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int k = k0 + 2 * u + khalf;
        const float* arow = At + min(k, K - 1) * LDP + l31;
        const float bsel = (k < K) ? bcur[u] : 0.f;  // K not a multiple of 2: the odd tail row
#pragma unroll
        for (int i = 0; i < MI; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[32 * i], bsel, acc[i], 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) bcur[u] = bnext[u];
    }

    // ---- epilogue: C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    if constexpr (RC) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = 32 * i + (r & 3) + 8 * (r >> 2) + 4 * khalf;
          ep.count(rowtab, row, cv && q0 + row < Q, acc[i][r]);
        }
    } else if (cv) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int q = q0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * khalf;
          if (q < Q) ep(t, q, col, N, acc[i][r]);
        }
    }
  }
  if constexpr (RC) {
    __syncthreads();   // (every wave arrives: the loop above is left by a wave-uniform break or by its bound)
    ep.flush(rowtab, q0, QP, tid);
  }
}


// The same arithmetic for SMALL maps (the attention masks of the coarse levels: 23x40 and 46x80 pixels, K = 256, 100 rows:
// 5-19 MB per launch), where the chunked kernel above is a chain of latencies -- stage A, barrier, then eight times
// "request 16 rows, run 16 MFMAs": 29 / 44 us for what the memory system delivers in a few.  ONE SHOT: a wave requests all
// 128 k-row pairs of its 32 columns at once (128 registers), A is requested in front of them and committed to LDS while
// they fly, and the 128 MFMAs then run back to back as the rows arrive (the hardware returns loads in order; every MFMA
// waits for exactly its own row).  Same k order, same fmaf chain: bit-identical to skinny_gemm_f32<1>.
template <typename Epilogue>
__global__ __launch_bounds__(MD_THREADS, 1) void skinny_gemm_f32_oneshot(const float* __restrict__ A,  // [T,Q,256]
                                                                          const float* __restrict__ B,  // [T,256,N]
                                                                          int Q, int N, int tiles_per_block, Epilogue ep) {
  constexpr int K = 256, QP = 32, LDP = QP + 1, NL = K / 2;
  constexpr bool RC = CountsRows<Epilogue>::value;
  extern __shared__ __attribute__((aligned(16))) float At[];  // [K][LDP]
  int frame = blockIdx.z;
  if constexpr (RC) frame *= ep.t_step;
  const int t = frame;
  const int q0 = blockIdx.y * QP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int khalf = lane >> 5, l31 = lane & 31;
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(B + (long long)t * K * N), 0, (int)((long long)K * N * 4), 0x00020000);
  int* rowtab = nullptr;   // [QP][2], row-counting epilogues only
  if constexpr (RC) {
    rowtab = reinterpret_cast<int*>(At + K * LDP);
    if (tid < 2 * QP) rowtab[tid] = 0;
  }

  // ---- A^T of rows q0 .. q0+31: requested first (16 loads per thread, coalesced along k) ...
  constexpr int NA = QP * K / MD_THREADS;
  float areg[NA];
  {
    const float* At_src = A + ((long long)t * Q) * K;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = tid + i * MD_THREADS, k = idx & (K - 1), q = idx >> 8;
      areg[i] = At_src[(long long)min(q0 + q, Q - 1) * K + k];     // rows past Q: a copy of the last row, never stored
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  float b[NL];
  auto request = [&](int tile) __attribute__((always_inline)) {
    const int col = min((blockIdx.x * tiles_per_block + tile) * MD_BLOCK_N + wave * MD_WAVE_N + l31, N - 1);
    const int voff = (col + khalf * N) * 4;
#pragma unroll
    for (int u = 0; u < NL; ++u) b[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, (2 * u) * N * 4, 0));
  };
  // ... then the first tile's rows of B, then A goes to LDS (waits for the A loads only: they are the oldest)
  request(0);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int idx = tid + i * MD_THREADS, k = idx & (K - 1), q = idx >> 8;
    At[k * LDP + q] = areg[i];
  }
  __syncthreads();

  const float* arow = At + khalf * LDP + l31;
  for (int tile = 0; tile < tiles_per_block; ++tile) {
    const int col0 = (blockIdx.x * tiles_per_block + tile) * MD_BLOCK_N + wave * MD_WAVE_N;
    if (col0 >= N) break;                    // wave-uniform
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int u = 0; u < NL; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[2 * u * LDP], b[u], acc, 0, 0, 0);
    const int col = col0 + l31;
    if (tile + 1 < tiles_per_block) request(tile + 1);   // (uniform) the next tile's rows fly under this tile's stores
    if constexpr (RC) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * khalf;
        ep.count(rowtab, row, col < N && q0 + row < Q, acc[r]);
      }
    } else if (col < N) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q = q0 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
        if (q < Q) ep(t, q, col, N, acc[r]);
      }
    }
  }
  if constexpr (RC) {
    __syncthreads();   // (every wave arrives: the loop above is left by a wave-uniform break or by its bound)
    ep.flush(rowtab, q0, QP, tid);
  }
}

// Rows of A per block tile, in blocks of 32: 128 rows when Q is large, else the smallest multiple of 32 covering Q -- unless that
// leaves most of the chip idle: the attention-mask maps of the coarse levels (23x40, 46x80) have 4 / 15 column tiles per frame, i.e.
// 20 / 75 workgroups at 128 rows per workgroup, each running 512 dependent MFMAs per wave (measured 57-71 us for a 5-20 MB
// problem: pure latency).  Fewer rows per workgroup = more workgroups and proportionally shorter MFMA chains; B is
// re-read from L2 once per row block, which is noise at these sizes.
inline int skinny_row_blocks(int T, int Q, long long N) {
  const long long ctiles = (N + MD_BLOCK_N - 1) / MD_BLOCK_N;
  int MI = (Q + 31) / 32;
  if (MI > 4) MI = 4;
  while (MI > 1 && ctiles * ((Q + 32 * MI - 1) / (32 * MI)) * T < 192) --MI;
  if (MI == 3 && (Q + 63) / 64 == (Q + 95) / 96) MI = 2;   // same number of row blocks with less padding
  return MI;
}

// bytes of dynamic LDS of a block tile of 32 * MI rows: the A tile [K][32 MI + 1] and, for a row-counting epilogue, its table
template <typename Epilogue>
inline size_t skinny_lds_bytes(int MI, int K) {
  const int QP = 32 * MI;
  return (size_t)K * (QP + 1) * sizeof(float) + (CountsRows<Epilogue>::value ? 2 * QP * sizeof(int) : 0);
}
constexpr size_t SKINNY_LDS_MAX = 160 * 1024;

// T = the frames the grid walks (a row-counting epilogue maps grid frame z to frame z * t_step of A and B)
template <typename Epilogue>
static int launch_skinny(const float* A, const float* B, int T, int Q, int K, long long N,
                         Epilogue ep, hipStream_t st, const char* what) {
  if (T == 0 || Q == 0 || N == 0) return UNIVS_OK;
  const long long ctiles = (N + MD_BLOCK_N - 1) / MD_BLOCK_N;
  const int MI = skinny_row_blocks(T, Q, N);
  const int QP = 32 * MI;
  const int qtiles = (Q + QP - 1) / QP;
  // amortise the A staging and balance the grid: just under one block per CU (256 CUs) when the
  // problem is large enough, one tile per block otherwise
  long long tpb = (ctiles * qtiles * T + 255) / 256;
  if (tpb < 1) tpb = 1;
  if (tpb > 16) tpb = 16;
  if ((long long)K * N * 4 >= (1LL << 31)) {
    set_error("%s: K*N too large for a 32-bit buffer range", what);
    return UNIVS_ERR_INVALID_ARGUMENT;
  }
  const long long gx = (ctiles + tpb - 1) / tpb;
  const size_t lds = skinny_lds_bytes<Epilogue>(MI, K);
  if (lds > SKINNY_LDS_MAX) {
    set_error("%s: K=%d too large for the LDS-resident A tile", what, K);
    return UNIVS_ERR_INVALID_ARGUMENT;
  }
  dim3 grid((unsigned)gx, (unsigned)qtiles, (unsigned)T), block(MD_THREADS);
  if (MI == 1 && K == 256 && config().mask_decode_chunked == 0) {   // small maps: every row of B requested at once
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&skinny_gemm_f32_oneshot<Epilogue>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((skinny_gemm_f32_oneshot<Epilogue>), grid, block, lds, st, A, B, Q, (int)N, (int)tpb, ep);
    return check_launch(what);
  }
#define UNIVS_LAUNCH_MI(mi)                                                                         \
  do {                                                                                              \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&skinny_gemm_f32<mi, Epilogue>),            \
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                      \
    hipLaunchKernelGGL((skinny_gemm_f32<mi, Epilogue>), grid, block, lds, st, A, B, Q, K, N,        \
                       (int)tpb, ep);                                                               \
  } while (0)
  switch (MI) {
    case 1: UNIVS_LAUNCH_MI(1); break;
    case 2: UNIVS_LAUNCH_MI(2); break;
    case 3: UNIVS_LAUNCH_MI(3); break;
    default: UNIVS_LAUNCH_MI(4); break;
  }
#undef UNIVS_LAUNCH_MI
  return check_launch(what);
}

}  // namespace univs
