/* libunivs_hip.so, ninth header: the first-frame masks of a video-object-segmentation video at the model's input size.  The eight other
 * headers are pinned symbol by symbol, so this entry has a header of its own.  Same library, same conventions: plain pointers and sizes,
 * device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_* return codes and univs_last_error() of
 * univs_hip.h. */
#ifndef UNIVS_PROMPTS_HIP_H
#define UNIVS_PROMPTS_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Pillow's NEAREST resize of run-length coded masks, and the boxes of the results (csrc/mask_prompt_resize.hip) -------------------------
 * The N masks of a video, all H x W, come as their cumulative column-major run boundaries back to back (the `Runs` layout of
 * univs_amd/evaluation/vis_counts.py): mask m owns bounds[starts[m] : starts[m + 1]], its run k covers the pixels [b_{k-1}, b_k) of the
 * column-major plane with b_{-1} = 0, odd runs are foreground, the last boundary is H W.  starts[m + 1] == starts[m]: the mask is
 * absent.  bounds: int32 [n_bounds], starts: int32 [N + 1], both on the device.
 * masks: uint8 [N, Ho, Wo], masks[m, yo, xo] = source pixel (ty[yo], tx[xo]) of mask m as 0 / 1 -- with the tables of
 * univs_amd/data/resize_rule.py (`nearest_table`: Pillow's running float64 sum, computed by the caller) the bytes of
 * `PIL.Image.fromarray(mask).resize((Wo, Ho), Image.NEAREST)`; an absent mask gives a zero plane.  ty: int32 [Ho] non-decreasing,
 * tx: int32 [Wo], on the device; the library does no floating-point arithmetic and keeps no table.
 * boxes: int32 [N, 4] = {x0, y0, x1 + 1, y1 + 1} with x0 / x1 the first / last column and y0 / y1 the first / last row of masks[m] that
 * holds a 1 (what detectron2's `BitMasks.get_bounding_boxes` returns, before its cast to float32), zeros for an empty or absent mask.
 * N < 0, n_bounds < 0, or H, W, Ho or Wo < 1 is an invalid argument; N == 0 is success and launches nothing.  A table entry outside
 * [0, n_in) is clamped before use, starts to [0, n_bounds], and no boundary beyond a mask's slice is read: bad tables, starts or
 * boundaries cost wrong pixels, never an address outside the inputs.
 * Covered: H W < 2^31, n_bounds < 2^31, N Ho Wo < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: per annotated object `mask_util.decode`, `ResizeTransform.apply_segmentation` (`PIL.Image.resize(NEAREST)` on one host
 * core), the stack of `annotations_to_instances` and `BitMasks.get_bounding_boxes` (dataset_mapper_uni_vid.py:456-486).  detectron2
 * is restated from its documented behaviour, Pillow is pinned bit for bit (tests/test_prompt_masks_gpu.py). */
int univs_resize_rle_masks_u8(const int32_t* bounds, const int32_t* starts, long long n_bounds, int N, int H, int W, const int32_t* ty,
                              const int32_t* tx, int Ho, int Wo, uint8_t* masks, int32_t* boxes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_PROMPTS_HIP_H */
