/* libunivs_hip.so, third header: entries in which a consumer applies, while it loads its operand, a transform that used to be a launch
 * and a tensor of its own.  Same library and conventions as include/univs_hip.h (whose symbols are pinned one by one in
 * tests/capi_signatures.txt): plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the
 * UNIVS_* return codes and univs_last_error(). */
#ifndef UNIVS_FUSED_HIP_H
#define UNIVS_FUSED_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 1 x 1 convolution with the operand's layout and normalisation folded in (csrc/gemm_f16x3_stream.hip) -------------------------------
 * y [T, Cout, H, W] = conv2d(x', w [Cout, Cin, 1, 1], bias) with wp / winv the split of w as for univs_conv1x1_presplit_f32.
 *   channels_last == 0: x is [T, Cin, H, W]; != 0: x is [T, H, W, Cin] (what a token tensor [T, H W, Cin] is) -- no NCHW copy is needed.
 *   affine == NULL: x' = x, and the result is univs_conv1x1_presplit_f32's bit for bit, in either layout.
 *   affine [T * Cin][2]: the (scale, bias) pairs univs_group_norm_affine_f32 writes for the NCHW tensor; x' = max(fma(x, scale, bias), 0) =
 *     relu(GroupNorm(x)), the very expression of univs_group_norm_f32(relu = 1), so the result is that of the convolution of the
 *     materialised tensor bit for bit.  Needs H W >= 256, Cin <= 1024, and passes of at most 64 output features (Cout <= 64, or a
 *     Cout the planner cuts into such passes) or, with Cin % 128 == 0, of exactly 128 (Cout % 128 == 0).
 * bias may be NULL.  Covered as univs_conv1x1_presplit_f32: Cin % 96 == 0 or % 128 == 0, Cout % 16 == 0, T H W >= 4096, 16-byte aligned
 * pointers; else UNIVS_ERR_NOT_IMPLEMENTED, before any launch.
 * Replaces: a transpose to NCHW in front of, or a GroupNorm + ReLU pass between, the convolutions of the pixel decoder
 * (mask2former/modeling/pixel_decoder/msdeformattn.py:214-232, :352-353). */
int univs_conv1x1_fused_presplit_f32(const float* x, int channels_last, const float* affine, const void* wp, const float* winv,
                                     const float* bias, int T, int Cin, int Cout, int H, int W, float* y, void* stream);

/* ---- attention core whose key-segment merge happens inside the out-projection (csrc/cross_attn.hip, csrc/small_linear.hip) ------------------
 * univs_cross_attention_f32 is two launches: the partial results of every key segment, then their merge into out [L, N, E].  These two
 * entries are the same partials and the few-rows Linear of univs_small_linear_presplit_f32 reading them: a slot of its operand tile is
 * merged from the segments (the expression of the merge kernel, one inline function for both) instead of loaded, so the merge launch and
 * the [L, N, E] tensor disappear and y is, bit for bit, univs_small_linear_presplit_f32(univs_cross_attention_f32(...)).
 *
 * univs_cross_attention_partials_f32: arguments and coverage of univs_cross_attention_flagged_f32 without `out`; workspace of
 * univs_cross_attention_workspace(L, S, N, H) floats.  *plan (a HOST int, written before the entry returns) = the launch it chose:
 * segments + 65536 * query blocks per wave, the packing of UnivsConfig.xattn_segments; 0 where nothing was launched. */
int univs_cross_attention_partials_f32(const float* q, const float* k, const float* v, const uint8_t* mask, const uint32_t* mask_row_flags,
                                       uint32_t mask_generation, int L, int S, int N, int H, int head_dim, int ldq, int ldk, int ldv,
                                       float scale, float* workspace, int* plan, void* stream);

/* y [L * N, n_out] = (attention output [L, N, 32 H], row q * N + n) W[f_off : f_off + n_out]^T + bias [+ residual] [-> LayerNorm], the
 * attention output merged from `workspace` as `plan` lays it out (workspace_floats: its size, checked against the plan).  The other
 * arguments as univs_small_linear_presplit_f32 (no x_add, no ReLU, no transposed store).  Covered: H <= 8, n_out % 16 == 0,
 * f_off % 4 == 0, with a LayerNorm n_out == 256, L N <= 1 048 560, 16-byte aligned pointers; else UNIVS_ERR_NOT_IMPLEMENTED.
 * Replaces: the tail of nn.MultiheadAttention -- the concatenation of the heads and out_proj -- with the decoder layer's residual and
 * LayerNorm (univs/modeling/transformer_decoder/transformer_layers.py:42-46, :106-110). */
int univs_small_linear_merged_presplit_f32(const float* workspace, long long workspace_floats, int plan, int L, int N, int H, const void* wp,
                                           const float* winv, const float* bias, int n_w, int f_off, const float* residual,
                                           const float* ln_weight, const float* ln_bias, float ln_eps, int n_out, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_FUSED_HIP_H */
