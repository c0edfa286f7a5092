// The test-time resize of decoded frames (include/univs_frames_hip.h): Pillow's 8-bit bilinear, bit for bit, from interleaved uint8
// [T, Hi, Wi, 3] to the planar uint8 [T, 3, Ho, Wo] the drivers take.  The reference does this per frame on a host core
// (`ResizeShortestEdge` -> `PIL.Image.resize`, then a transpose: dataset_mapper_uni_vid.py:423-433).
//
// Pillow's resize is two integer passes, horizontal then vertical, each
//     out = clamp((2^21 + sum_{k < count[i]} coef[i][k] * in[first[i] + k]) >> 22, 0, 255)
// with the image uint8 in between (univs_amd/data/resize_rule.py states the tables).  The tables are arguments: there is no floating
// point here.  The sums are formed in 32 bits: the coefficients of an output sum to 2^22 up to their rounding and a pixel is at most
// 255, so a sum stays below 2^30 + 2^21 (unsigned arithmetic, so that a table that breaks this wraps and does not overflow).
//
// A workgroup of 256 threads owns FR_TH x FR_TW = 16 x 64 output pixels of one frame, all three channels.  It copies the tile's slices
// of the six tables into LDS, clamped so that no tap can leave the source whatever the tables hold.  Pass 1: for the source rows
// [first_y(tile's first row), first_y + count_y (tile's last row)) a wave takes a row, a lane an output column; it reads its taps'
// three interleaved bytes from global memory (neighbouring lanes read overlapping spans of one row: L1 hits) and writes the three
// rounded results into three LDS planes [rows][64] of uint8 -- the intermediate rounding is part of the answer.  Pass 2: a lane takes
// four neighbouring columns of one output row of one plane, reads a dword of four stage pixels per tap, and stores the four results as
// one dword where the address is 4-byte aligned (with Wo % 4 != 0 that is one row in four) and as bytes elsewhere and at the ragged
// right edge.  An axis that keeps its size has no pass in Pillow; here it runs with the one tap (first = i, coef = 2^22), which is the
// identity exactly, and its tables are not read.
//
// LDS: the stage is 3 x rows x 64 bytes with rows <= ceil(15 Hi / Ho) + ksize_y + 1: 70 rows, 13.1 KB, at the coverage edge (a down-scale by
// 4, ksize 9), 29 rows, 5.4 KB, for 1080p -> 720p; the tables take 3.4 KB.  Pass 1 is recomputed for the source rows two vertically neighbouring
// tiles share: (ksize_y - 1) of about 16 Hi / Ho + ksize_y rows.  Nothing about this kernel's speed is claimed here; tools/frames_bench.py
// measures it.
#include <stdint.h>

#include "launchers.h"

namespace univs {

constexpr int FR_TW = 64;                                          // output columns of a tile: one per lane in pass 1
constexpr int FR_TH = 16;                                          // output rows of a tile
constexpr int FR_KMAX = 9;                                         // taps per output: a down-scale up to 4
constexpr int FR_BITS = 22;                                        // Pillow's PRECISION_BITS for 8-bit images

// Pillow's clip8 of a sum.  The sum of a valid table is never negative (bilinear weights are not), so the clamp from below is the
// unsigned shift itself.  Written on unsigned values on purpose: for clamp(int >> 22, 0, 255) of two sums packed into one word hipcc
// (ROCm 7.2) selects v_ashr_pk_u8_i32 and then ORs bytes 2 and 3 into its result as if bits 31:16 were zero; on the MI355X they keep what
// the destination register held, and the third and fourth pixel of a lane came out OR-ed with an old partial sum (DESIGN.md section 3,
// toolchain hazards).
__device__ __forceinline__ unsigned fr_round(unsigned acc) { return min(acc >> FR_BITS, 255u); }

__global__ __launch_bounds__(256) void frame_resize_kernel(const unsigned char* __restrict__ src, int Hi, int Wi, int Ho, int Wo,
                                                           const int* __restrict__ first_x, const int* __restrict__ count_x,
                                                           const int* __restrict__ coef_x, int ksx, const int* __restrict__ first_y,
                                                           const int* __restrict__ count_y, const int* __restrict__ coef_y, int ksy,
                                                           int swap_rb, int rows_cap, int tiles_x, int tiles_y,
                                                           unsigned char* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fr_stage[];   // [3][rows_cap][FR_TW]
  __shared__ int s_cx[FR_TW * FR_KMAX], s_cy[FR_TH * FR_KMAX], s_fx[FR_TW], s_nx[FR_TW], s_fy[FR_TH], s_ny[FR_TH];
  const int tid = threadIdx.x;

  int blk = blockIdx.x;
  const int tx = blk % tiles_x;
  blk /= tiles_x;
  const int ty = blk % tiles_y, t = blk / tiles_y;
  const int x0 = tx * FR_TW, y0 = ty * FR_TH;
  const bool same_x = Wi == Wo, same_y = Hi == Ho;

  // ---- the tile's tables; columns and rows beyond the image repeat the last one (computed, never stored) ------------------------------
  if (tid < FR_TW) {
    const int x = min(x0 + tid, Wo - 1);
    const int f = min(max(same_x ? x : first_x[x], 0), Wi - 1);
    s_fx[tid] = f;
    s_nx[tid] = min(max(same_x ? 1 : count_x[x], 0), min(ksx, Wi - f));
  } else if (tid < FR_TW + FR_TH) {
    const int yl = tid - FR_TW, y = min(y0 + yl, Ho - 1);
    const int f = min(max(same_y ? y : first_y[y], 0), Hi - 1);
    s_fy[yl] = f;
    s_ny[yl] = min(max(same_y ? 1 : count_y[y], 0), min(ksy, Hi - f));
  }
  for (int i = tid; i < FR_TW * ksx; i += 256) {
    const int xl = i / ksx, k = i - xl * ksx;
    s_cx[i] = same_x ? (k == 0 ? 1 << FR_BITS : 0) : coef_x[(size_t)min(x0 + xl, Wo - 1) * ksx + k];
  }
  for (int i = tid; i < FR_TH * ksy; i += 256) {
    const int yl = i / ksy, k = i - yl * ksy;
    s_cy[i] = same_y ? (k == 0 ? 1 << FR_BITS : 0) : coef_y[(size_t)min(y0 + yl, Ho - 1) * ksy + k];
  }
  __syncthreads();

  // ---- the source rows the tile's output rows read: [r0, r0 + nrows), within the stage and the image --------------------------------
  const int yl_last = min(y0 + FR_TH, Ho) - 1 - y0;
  const int r0 = s_fy[0];
  const int nrows = min(max(s_fy[yl_last] + s_ny[yl_last] - r0, 1), min(rows_cap, Hi - r0));

  // ---- pass 1: a wave per source row, a lane per output column, three channels; T Hi Wi 3 < 2^31 ------------------------------------
  {
    const int xl = tid & (FR_TW - 1);
    const int f = s_fx[xl], n = s_nx[xl];
    const int* cx = s_cx + xl * ksx;                               // (ksx is odd: the lanes' coefficients fall on distinct banks)
    unsigned char* p0 = fr_stage + (swap_rb ? 2 : 0) * rows_cap * FR_TW + xl;   // where source channel 0 goes
    unsigned char* p1 = fr_stage + rows_cap * FR_TW + xl;
    unsigned char* p2 = fr_stage + (swap_rb ? 0 : 2) * rows_cap * FR_TW + xl;
    for (int row = tid >> 6; row < nrows; row += 4) {
      const unsigned char* p = src + ((t * Hi + r0 + row) * Wi + f) * 3;
      unsigned a0 = 1u << (FR_BITS - 1), a1 = a0, a2 = a0;
      for (int k = 0; k < n; ++k) {
        const unsigned w = (unsigned)cx[k];
        a0 += w * p[3 * k];
        a1 += w * p[3 * k + 1];
        a2 += w * p[3 * k + 2];
      }
      p0[row * FR_TW] = (unsigned char)fr_round(a0);
      p1[row * FR_TW] = (unsigned char)fr_round(a1);
      p2[row * FR_TW] = (unsigned char)fr_round(a2);
    }
  }
  __syncthreads();

  // ---- pass 2: a lane per four columns of an output row of a plane; each of the three rounds of 256 lanes is one plane ---------------
  for (int item = tid; item < 3 * FR_TH * (FR_TW / 4); item += 256) {
    const int q = item & (FR_TW / 4 - 1), yl = (item / (FR_TW / 4)) & (FR_TH - 1), c = item / (FR_TH * FR_TW / 4);
    const int x = x0 + 4 * q, y = y0 + yl;
    if (x >= Wo || y >= Ho) continue;
    const int f = s_fy[yl] - r0, n = s_ny[yl];
    const int* cy = s_cy + yl * ksy;
    const unsigned char* col = fr_stage + c * rows_cap * FR_TW + 4 * q;
    unsigned a0 = 1u << (FR_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int k = 0; k < n; ++k) {
      const int r = min(max(f + k, 0), nrows - 1);                 // (a clamp only for tables that are not monotone)
      const unsigned w = (unsigned)cy[k];
      const unsigned d = *reinterpret_cast<const unsigned*>(col + r * FR_TW);
      a0 += w * (d & 255u);
      a1 += w * ((d >> 8) & 255u);
      a2 += w * ((d >> 16) & 255u);
      a3 += w * (d >> 24);
    }
    const unsigned v = fr_round(a0) | (fr_round(a1) << 8) | (fr_round(a2) << 16) | (fr_round(a3) << 24);
    unsigned char* o = out + (((size_t)t * 3 + c) * Ho + y) * Wo + x;
    if (x + 3 < Wo && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
      *reinterpret_cast<unsigned*>(o) = v;
    } else {
      for (int j = 0; j < 4 && x + j < Wo; ++j) o[j] = (unsigned char)(v >> (8 * j));
    }
  }
}

int resize_frames_u8(const unsigned char* src, int T, int Hi, int Wi, int Ho, int Wo, const int* first_x, const int* count_x,
                     const int* coef_x, int ksize_x, const int* first_y, const int* count_y, const int* coef_y, int ksize_y, int swap_rb,
                     unsigned char* out, hipStream_t st) {
  const long long tiles_x = (Wo + FR_TW - 1) / FR_TW, tiles_y = (Ho + FR_TH - 1) / FR_TH;
  if (ksize_x > FR_KMAX || ksize_y > FR_KMAX || 3LL * T * Hi * Wi >= (1LL << 31) || 3LL * T * Ho * Wo >= (1LL << 31) ||
      tiles_x * tiles_y * T >= (1LL << 31))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  // every source row one tile can read: (FR_TH - 1) scale between its first and last centre, a support on either side, the rounding
  const int rows_cap = Hi == Ho ? FR_TH : (int)(((long long)(FR_TH - 1) * Hi + Ho - 1) / Ho) + (ksize_y - 1) + 2;
  const size_t lds = (size_t)3 * rows_cap * FR_TW;
  hipLaunchKernelGGL(frame_resize_kernel, dim3((unsigned)(tiles_x * tiles_y * T)), dim3(256), lds, st, src, Hi, Wi, Ho, Wo, first_x, count_x,
                     coef_x, ksize_x, first_y, count_y, coef_y, ksize_y, swap_rb, rows_cap, (int)tiles_x, (int)tiles_y, out);
  return check_launch("resize_frames_u8");
}

}  // namespace univs
