/* libunivs_hip.so, seventh header: Swin window attention that computes q, k, v itself.  The six other headers (univs_hip.h,
 * univs_eval_hip.h, univs_fused_hip.h, univs_pvos_hip.h, univs_semantic_hip.h, univs_encoder_hip.h) are pinned symbol by symbol, so this
 * entry has a header of its own.  Same library, same conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t,
 * NULL = the default stream) last, the UNIVS_* return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_SWIN_HIP_H
#define UNIVS_SWIN_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the qkv Linear inside image-mode window attention (csrc/window_attn_qkv.hip) -----------------------------------------------------
 *   out = window_attention_image(x W_qkv^T + qkv_bias)      x [B, H*W, C] normalised tokens in image order, out [B, H*W, C]
 * in ONE launch: the [B, H*W, 3C] tensor between the qkv Linear and the attention core is never written.
 * wp / winv: the split image and inverse row scales of qkv.weight [3C, C] (univs_presplit_weights_f32, mode 0); qkv_bias [3C] or NULL;
 * rel_bias [nH, ws*ws, ws*ws]; shift_mask [nW, ws*ws, ws*ws] or NULL (shift == 0 ignores it); scale multiplies q.
 * The result has the bits of univs_linear_resident_presplit_f32 followed by univs_window_attention_image_mma(..., UNIVS_MMA_F16X3) on the
 * materialised tensor (the same arithmetic: the three-product pass kernels' k-step, then the same attention text).
 * Covered: ws == 7, C == 32 nH in {96, 192} (head_dim 32; Swin-T/S stages 1 and 2), x and wp 16-byte aligned, the other pointers 4-byte
 * aligned, B H W C 4 < 2^31 - 1; else UNIVS_ERR_NOT_IMPLEMENTED, before any launch.  B < 0, H, W, ws, nH or C < 1 or shift outside
 * [0, ws) is an invalid argument, as is a NULL x, wp, winv, rel_bias or out with B > 0.
 * Replaces: `qkv = self.qkv(x)` with the attention core behind it (swin.py:137-168) and the pad / roll / partition / reverse / crop
 * around them (:252-284). */
int univs_swin_window_attention_qkv_presplit_f32(const float* x, const void* wp, const float* winv, const float* qkv_bias,
                                                 const float* rel_bias, const float* shift_mask, int B, int H, int W, int ws, int shift,
                                                 int nH, int C, float scale, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_SWIN_HIP_H */
