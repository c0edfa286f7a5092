/* libunivs_hip.so, sixth header: the head of a deformable-encoder layer.  The five other headers (univs_hip.h, univs_eval_hip.h,
 * univs_fused_hip.h, univs_pvos_hip.h, univs_semantic_hip.h) are pinned symbol by symbol, so this entry has a header of its own.  Same
 * library, same conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the
 * UNIVS_* return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_ENCODER_HIP_H
#define UNIVS_ENCODER_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- two Linears on one read of x (csrc/linear_pair_f16x3.hip) ---------------------------------------------------------------------------
 *   y_a = x W_a^T + bias_a                               x [M, K]
 *   y_b = (x + add[row % add_rows]) W_b^T + bias_b       add [add_rows, K]
 * in ONE launch: MSDeformAttn's value_proj on `src` and its merged sampling-offset / attention-weight projection on `src + pos`, pos one
 * frame's table.  The sum is formed in registers (one fp32 add per element), `src + pos` is never a tensor.
 * wp_* / winv_*: the weights' split images and inverse row scales (univs_presplit_weights_f32, mode 0), W_a [N_a, K], W_b [N_b, K];
 * bias_* [N_*] or NULL.  Outputs column-blocked as univs_linear_blocked_presplit_f32 writes them:
 * y_* [M / rows_per_batch][N_* / col_block_*][rows_per_batch][col_block_*].  Each output has the bits of that entry on the materialised
 * operand (the same arithmetic: three fp16 products on two-part splits, running row scale).
 * Covered: K == 256, add_rows == rows_per_batch, M a multiple of it, N_* a multiple of col_block_* and col_block_* of 4, N_a in
 * passes of 113 .. 128 features and N_b in passes of 81 .. 96 as csrc/gemm_plan.h: plan_f16x3_pair divides them (the one kernel built;
 * the model's 256 = 2 x 128 and 288 = 3 x 96), 16-byte aligned pointers, M max(K, N_a, N_b) 4 < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before any
 * launch.  M, N_*, K, add_rows, rows_per_batch or col_block_* < 1 is an invalid argument, as is a NULL x, add, image, scale or output.
 * Replaces: `value = self.value_proj(input_flatten)` with `self.sampling_offsets(query)` / `self.attention_weights(query)` and the
 * `with_pos_embed(src, pos)` in front of them (ops/modules/ms_deform_attn.py:95-104, msdeformattn.py:61-63). */
int univs_encoder_linear_pair_presplit_f32(const float* x, const float* add, long long add_rows, const void* wp_a, const float* winv_a,
                                           const float* bias_a, int N_a, int col_block_a, float* y_a, const void* wp_b,
                                           const float* winv_b, const float* bias_b, int N_b, int col_block_b, float* y_b, long long M,
                                           int K, long long rows_per_batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_ENCODER_HIP_H */
