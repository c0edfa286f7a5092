/* libunivs_hip.so, eighteenth header: causal self-attention over packed sequences of unequal length -- the attention core of the CLIP
 * text tower on its real tokens only.  The seventeen other headers are pinned symbol by symbol, so this entry has a header of its own.
 * Same library, same conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last,
 * the UNIVS_* return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_TEXT_HIP_H
#define UNIVS_TEXT_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- out[i] = softmax(scale q_i . k_{j <= i}) v_{j <= i} per sequence and head (csrc/text_attn.hip) -----------------------------------------
 * qkv: float32 [Ntok, 3 E], the packed in-projection (q | k | v, heads of d = E / heads channels side by side) of all sequences' kept
 * tokens; sequence s owns rows start[s] .. start[s + 1].  start: int32 [S + 1] ON THE DEVICE.  out: float32 [Ntok, E]; the rows of
 * every sequence are written, nothing else.  Lmax: no sequence is longer (it sizes the LDS image of a head's keys and values).
 * The kernel trusts no entry of `start`: a length is clamped to [0, Lmax] and the first row so that the sequence lies inside the
 * tensors; a caller that wants an error for a wrong table checks it on the host, where it built it (text_ops.check_start).
 * fp32 throughout: fmaf chains, expf(score - rowmax), one division per row.  qkv is read once and out written once.
 * S < 0, Ntok < 0, E < 1, heads < 1, E % heads != 0 or Lmax < 1 is an invalid argument; S == 0 or Ntok == 0 is success and launches
 * nothing.
 * Covered: d in {16, 32, 64}, Lmax <= 128, Ntok 3 E < 2^31, S heads < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: between in_proj and out_proj of nn.MultiheadAttention(E, heads) under attn_mask = triu(1) (CLIP's
 * build_attention_mask), for sequences whose padding is never computed. */
int univs_text_attention_f32(const float* qkv, const int* start, int S, long long Ntok, int E, int heads, int Lmax, float scale, float* out,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_TEXT_HIP_H */
