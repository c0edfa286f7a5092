/* libunivs_hip.so, fifteenth header: the prompts of a video-object-segmentation video straight from the id maps of its annotation PNGs.
 * The fourteen other headers are pinned symbol by symbol, so these two entries have a header of their own.  Same library, same
 * conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_* return
 * codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_IDMAP_HIP_H
#define UNIVS_IDMAP_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- which values the id maps hold, how often and where (csrc/idmap_prompts.hip) ----------------------------------------------------------
 * ids: uint8 [F, H, W], a pixel's value is its object's id (the pixels of an indexed annotation PNG).
 * count: int32 [F, 256], count[f, v] = the pixels of frame f with value v.
 * box: int32 [F, 256, 4] = {x0, y0, x1 + 1, y1 + 1} with x0 / x1 the first / last column and y0 / y1 the first / last row of frame f
 * that holds value v, at the source size; zeros for a value that is absent.  Both are written in full, in one pass over the bytes.
 * F < 0, H < 1 or W < 1 is an invalid argument; F == 0 is success and launches nothing.
 * Covered: F H W < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: per frame `np.unique(mask)`, and per object `mask == obj_id`, `.any()`, the two `np.any` / `np.where` scans of
 * `bounding_box` and `np.sum` in the data sets' converters to YouTube-VIS json (datasets/data_utils/convert_*_to_cocovid_val.py). */
int univs_idmap_census_u8(const uint8_t* ids, int F, int H, int W, int32_t* count, int32_t* box, void* stream);

/* ---- the listed objects' masks at the model's input size, and their boxes (csrc/idmap_prompts.hip) ------------------------------------------
 * Object n of N is value[n] in frame frame[n] of ids (uint8 [F, H, W] as above); frame, value: int32 [N] on the device, frame
 * non-decreasing (a frame's objects are one slice of the list).
 * masks: uint8 [N, Ho, Wo], masks[n, yo, xo] = (ids[frame[n], ty[yo], tx[xo]] == value[n]) as 0 / 1 -- with the tables of
 * univs_amd/data/resize_rule.py (`nearest_table`: Pillow's running float64 sum, computed by the caller) the bytes of
 * `PIL.Image.fromarray(ids[frame[n]] == value[n]).resize((Wo, Ho), Image.NEAREST)`: NEAREST is a gather, so comparing after it is
 * comparing before it.  ty: int32 [Ho], tx: int32 [Wo], on the device; the library does no floating-point arithmetic and keeps no table.
 * boxes: int32 [N, 4] = {x0, y0, x1 + 1, y1 + 1} of masks[n] as in univs_resize_rle_masks_u8 (include/univs_prompts_hip.h), zeros for an
 * empty mask.  A value may be listed twice: both planes and boxes are written.  A listed value that does not occur in its frame gives a
 * zero plane and a zero box.
 * N < 0, F < 0, F == 0 with N > 0, or H, W, Ho or Wo < 1 is an invalid argument; N == 0 is success and launches nothing.  frame is
 * clamped to [0, F), value to [0, 255] and a table entry to [0, n_in) before use: bad entries cost wrong pixels (a frame list that goes
 * down: planes that are not written), never an address outside the inputs.
 * Covered: F H W < 2^31, N Ho Wo < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: the converters' per-object planes and run-length codes, and then per annotated object `mask_util.decode`,
 * `ResizeTransform.apply_segmentation`, the stack of `annotations_to_instances` and `BitMasks.get_bounding_boxes`
 * (dataset_mapper_uni_vid.py:456-486).  Pillow is pinned bit for bit (tests/test_idmap_prompts_gpu.py). */
int univs_idmap_prompts_u8(const uint8_t* ids, int F, int H, int W, const int32_t* frame, const int32_t* value, int N, const int32_t* ty,
                           const int32_t* tx, int Ho, int Wo, uint8_t* masks, int32_t* boxes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_IDMAP_HIP_H */
