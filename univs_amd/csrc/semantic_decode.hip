// The mask-quality counts of the semantic-feature decoder (univs_amd/inference/semantic_to_mask.py) without the logits.
//
// Reference semantics (semantic_feature_to_mask.py:9-12, :101-110): mask_logits = einsum("tnc,tchw->tnhw", mask_embed, mask_feats)
// transposed to [N, T, h, w] -- the whole stack, 3.5 GB at T = 300, N = 200, 90 x 160 --, then on mask_logits[:, ::temporal_stride]
//     (logit > 1).flatten(1).sum(-1) / (logit > -1).flatten(1).sum(-1).clamp(min=1)
// which only decides which rows are kept.  Here the logits of every temporal_stride-th frame are formed in the MFMA accumulators and
// compared there; what reaches memory is counts int32 [N, 2] = (|{logit > t_hi}|, |{logit > t_lo}|) per row, strict comparisons.
//
// The contraction is the one of the exact-f32 mask decode (skinny_gemm_f32.h: skinny_gemm_f32 / skinny_gemm_f32_oneshot, the same
// templates csrc/mask_decode.hip instantiates with its storing epilogues): a k-ordered fp32 fmaf chain per logit.  The rows the
// caller keeps are decoded afterwards by ops.mask_decode under the exact-f32 setting, so a counted logit and a stored logit are the
// same float and the counts are the stored logits' counts, exactly.
//
// The epilogue.  In the 32 x 32 MFMA result layout a register of a lane is one row at one column: lanes 0..31 hold row r at the 32
// columns of the wave tile, lanes 32..63 row r + 4.  One 64-lane ballot per register and threshold therefore is the two rows' bit
// masks; lane 0 and lane 32 each add their half's population count to the workgroup's LDS table [rows][2] (no add for a zero).  Clamped
// columns (past HW; the 32 columns of a wave tile can straddle it) and padded rows (past N: zeros or copies of the last row) are masked
// out of the ballot's predicate.  After the last tile every touched cell of the table goes to `counts` with one integer atomic: at
// most 2 x 128 per workgroup, contiguous in memory, against 128 MFMAs per wave and tile.  Integer sums: the result does not depend
// on the order.  `counts` is zeroed here, on the caller's stream.
#include "launchers.h"
#include "skinny_gemm_f32.h"

namespace univs {

struct CountRows {
  int* counts;      // [N, 2]
  int t_step;       // grid frame z is frame z * t_step
  float t_hi, t_lo;
  __device__ __forceinline__ void count(int* tab, int row, bool valid, float v) const {
    const unsigned long long hi = __ballot(valid && v > t_hi), lo = __ballot(valid && v > t_lo);
    const int lane = threadIdx.x & 63;
    if ((lane & 31) == 0) {                                          // lane 0: rows' lower half of the wave, lane 32: the upper
      const int nh = __popc((unsigned)(hi >> lane)), nl = __popc((unsigned)(lo >> lane));
      if (nh) atomicAdd(&tab[2 * row], nh);
      if (nl) atomicAdd(&tab[2 * row + 1], nl);
    }
  }
  // (a cell of a row past N stays zero: nothing is added beyond counts[2 N])
  __device__ __forceinline__ void flush(const int* tab, int q0, int rows, int tid) const {
    for (int i = tid; i < 2 * rows; i += MD_THREADS) {
      const int v = tab[i];
      if (v) atomicAdd(&counts[2 * q0 + i], v);
    }
  }
};

int semantic_quality_counts_f32(const float* mask_embed, const float* features, int T, int N, int C, int HW, int t_step, float t_hi,
                                float t_lo, int* counts, hipStream_t st) {
  const int frames = (T + t_step - 1) / t_step;                     // t = 0, s, 2 s, ... < T
  // a count is an int32; a frame of the features is one 32-bit buffer range; the grid's y and z; the A tile and the table in LDS
  if ((long long)frames * HW >= (1LL << 31) || (long long)C * HW * 4 >= (1LL << 31) || frames > 65535 || N > 65535 * 32 ||
      skinny_lds_bytes<CountRows>(skinny_row_blocks(frames, N, HW), C) > SKINNY_LDS_MAX)
    return UNIVS_ERR_NOT_IMPLEMENTED;
  const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * 2 * (size_t)N, st);
  if (e != hipSuccess) {
    set_error("semantic_quality_counts: memset failed: %s", hipGetErrorString(e));
    return UNIVS_ERR_LAUNCH;
  }
  return launch_skinny(mask_embed, features, frames, N, C, HW, CountRows{counts, t_step, t_hi, t_lo}, st, "semantic_quality_counts");
}

}  // namespace univs
