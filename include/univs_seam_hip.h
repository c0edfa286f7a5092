/* libunivs_hip.so, sixteenth header: the seams of a post-norm decoder layer -- two few-rows kernels of which the second reads nothing
 * but the first one's output, in one launch.  The fifteen other headers are pinned symbol by symbol, so these two entries have a header
 * of their own (they belong beside univs_small_linear_presplit_f32 and univs_small_mlp_presplit_f32 of univs_hip.h).  Same library, same
 * conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_* return
 * codes and univs_last_error() of univs_hip.h.  Every result has the bits of the launches it replaces. */
#ifndef UNIVS_SEAM_HIP_H
#define UNIVS_SEAM_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- out-projection + residual + LayerNorm, then the next sub-layer's first Linear (csrc/small_linear.hip: small_seam_kernel) ------------
 * t [M, Na] = LayerNorm(residual + x Wa^T + bias_a)             -- univs_small_linear_presplit_f32 with residual and LayerNorm
 * y [M, Nb] = act((t [+ add]) Wb[f_off : f_off + Nb]^T + bias_b) -- univs_small_linear_presplit_f32 on t with x_add = add
 * wpa / winv_a: the split of Wa [Na, Ka]; wpb / winv_b: the split of Wb [n_wb, Na] (univs_presplit_weights_f32); bias_a [Na], bias_b
 * [n_wb], ln_bias and add [M, Na] may be NULL; relu != 0: act = ReLU; add_features as in univs_small_linear_presplit_f32 (add enters
 * the output features below it only; 0: all).  t is handed to the second product through LDS, and stored.
 * M < 0, Nb < 0, n_wb < 1 or a feature range outside Wb is an invalid argument; M == 0 or Nb == 0 is success and launches nothing.
 * Covered: Ka == Na == 256, Nb % 256 == 0, f_off % 4 == 0, add_features % 32 == 0, M <= 1 048 560, 16-byte aligned pointers; else
 * UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: two launches at the seam between the sub-layers of a decoder layer -- the tail of the cross-attention and the packed
 * in-projection of the self-attention, the tail of the self-attention and linear1 + ReLU of the FFN
 * (univs/modeling/transformer_decoder/transformer_layers.py:42-46, :106-110, :150-166). */
int univs_small_seam_presplit_f32(const float* x, const void* wpa, const float* winv_a, const float* bias_a, const float* residual,
                                  const float* ln_weight, const float* ln_bias, float ln_eps, float* t, const float* add, const void* wpb,
                                  const float* winv_b, const float* bias_b, int n_wb, int f_off, long long M, int Ka, int Na, int Nb, int relu,
                                  int add_features, float* y, void* stream);

/* ---- univs_small_mlp_presplit_f32 with the end of the decoder layer in front of it (csrc/small_linear.hip: small_chain_kernel) ------------
 * pre_residual != NULL: the chain's input rows are x' = LayerNorm(x + pre_residual) (pre_ln_weight, pre_ln_bias [256], both needed),
 *   the bits of univs_layer_norm_f32 with a residual; x_out [M, 256] receives them (needed).  Else x' = x and the four are NULL.
 * side_wp != NULL: side_y [M, 256] = (x' [+ side_add]) Wside[side_f_off : side_f_off + 256]^T + side_bias, the bits of
 *   univs_small_linear_presplit_f32 on x' (side_wp / side_winv: the split of Wside [side_n_w, 256]; side_add [M, 256] and side_bias
 *   [side_n_w] may be NULL; side_f_off % 4 == 0).  Else the five pointers are NULL.
 * The other arguments, and y, as univs_small_mlp_presplit_f32 on x'.
 * Covered as univs_small_mlp_presplit_f32, with 16-byte aligned pointers; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: the FFN's `norm(tgt + linear2(.))` launch in front of a prediction head's decoder_norm + mask-embedding MLP, and the next
 * layer's cross-attention query projection behind it (transformer_layers.py:106-110, :164-166, :205-217). */
int univs_small_mlp_seam_presplit_f32(const float* x, const float* pre_residual, const float* pre_ln_weight, const float* pre_ln_bias,
                                      float pre_ln_eps, float* x_out, const float* side_add, const void* side_wp, const float* side_winv,
                                      const float* side_bias, int side_n_w, int side_f_off, float* side_y, int stages,
                                      const void* const* wp, const float* const* winv, const float* const* bias, const int* relu,
                                      const float* in_ln_weight, const float* in_ln_bias, float in_ln_eps, float* x_normed, long long M,
                                      int out_T, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_SEAM_HIP_H */
