/* libunivs_hip.so, fifth header: the mask-quality counts of the semantic-feature decoder.  The four other headers (univs_hip.h,
 * univs_eval_hip.h, univs_fused_hip.h, univs_pvos_hip.h) are pinned symbol by symbol, so this entry has a header of its own.  Same
 * library, same conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the
 * UNIVS_* return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_SEMANTIC_HIP_H
#define UNIVS_SEMANTIC_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- which rows of a semantic-extraction video are high-quality masks (csrc/semantic_decode.hip) -------------------------------------------
 * mask_embed: float32 [T, N, C], features: float32 [T, C, HW], both contiguous.  For the frames t = 0, t_step, 2 t_step, ... < T the
 * logits logit[n, t, p] = sum_c mask_embed[t, n, c] * features[t, c, p] are formed and compared; none is written.  counts: int32 [N, 2],
 * ZEROED BY THIS ENTRY on `stream`; counts[n] = (the number of walked logits of row n > t_hi, the number > t_lo), strict comparisons.
 * A logit is the k-ordered fp32 fmaf chain of univs_mask_decode_f32 under univs_mask_decode_set_impl(1) (the same kernel templates):
 * the counts are exactly those of the logits that entry stores.
 * T, N, C, HW or t_step < 1 is an invalid argument.  Covered: ceil(T / t_step) * HW < 2^31 (a count is an int32), C * HW * 4 < 2^31,
 * ceil(T / t_step) <= 65535, N <= 65535 * 32 and an A tile that fits the LDS (C <= 315 for any N; C <= 1239 for N <= 32); else
 * UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: the [N, T, h, w] logit stack, its `[:, ::temporal_stride]` view, the two boolean stacks and the two reductions of
 * `calculate_mask_quality_scores` (semantic_feature_to_mask.py:9-12, :101-110). */
int univs_semantic_quality_counts_f32(const float* mask_embed, const float* features, int T, int N, int C, int HW, int t_step, float t_hi,
                                      float t_lo, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_SEMANTIC_HIP_H */
