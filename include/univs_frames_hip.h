/* libunivs_hip.so, eighth header: the test-time resize of decoded frames.  The seven other headers are pinned symbol by symbol, so this
 * entry has a header of its own.  Same library, same conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t,
 * NULL = the default stream) last, the UNIVS_* return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_FRAMES_HIP_H
#define UNIVS_FRAMES_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Pillow's 8-bit bilinear resize of a stack of frames, interleaved in, planar out (csrc/frame_resize.hip) -------------------------------
 * src: uint8 [T, Hi, Wi, 3] (HWC, as an image file decodes), out: uint8 [T, 3, Ho, Wo], both contiguous, on the device.  The result is
 * `PIL.Image.resize((Wo, Ho), BILINEAR)` of every frame bit for bit: a horizontal pass, then a vertical pass, each
 *     out = clamp((2^21 + sum_{x < count[i]} coef[i * ksize + x] * in[first[i] + x]) >> 22, 0, 255)
 * in int32, the image uint8 between the two.  The tables are the caller's, int32 on the device: first_x / count_x [Wo], coef_x [Wo,
 * ksize_x], first_y / count_y [Ho], coef_y [Ho, ksize_y] (univs_amd/data/resize_rule.py: `resize_tables` states them); the library does
 * no floating-point arithmetic and keeps no table.  An axis that keeps its size (Wi == Wo, Hi == Ho) has no pass, as in Pillow: its
 * three tables are not read and may be NULL, its ksize must still be 3.  swap_rb != 0 writes source channel 2 to plane 0 and channel 0
 * to plane 2 (RGB files, a "BGR" model).
 * T, Hi, Wi, Ho or Wo < 1, or a ksize that is not 2 ceil(max(n_in / n_out, 1)) + 1 of its axis, is an invalid argument.  A table must
 * satisfy 0 <= first[i], first[i] + count[i] <= n_in, count[i] <= ksize; the kernel clamps what it reads from one that does not, so
 * such a table costs wrong pixels, never an address outside src.
 * Covered: ksize_x <= 9 and ksize_y <= 9 (every up-scale, a down-scale up to 4), T Hi Wi 3 < 2^31, T 3 Ho Wo < 2^31, and fewer than
 * 2^31 tiles of 16 x 64 output pixels; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: `ResizeShortestEdge` -> `ResizeTransform.apply_image` -> `PIL.Image.resize` per frame on the host, and the
 * `torch.as_tensor(image.transpose(2, 0, 1))` that follows it (dataset_mapper_uni_vid.py:423-433). */
int univs_resize_frames_u8(const uint8_t* src, int T, int Hi, int Wi, int Ho, int Wo, const int32_t* first_x, const int32_t* count_x,
                           const int32_t* coef_x, int ksize_x, const int32_t* first_y, const int32_t* count_y, const int32_t* coef_y,
                           int ksize_y, int swap_rb, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_FRAMES_HIP_H */
