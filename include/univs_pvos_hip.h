/* libunivs_hip.so, fourth header: the counts of the VIPOSeg panoptic-VOS scoring.  The three other headers (univs_hip.h,
 * univs_eval_hip.h, univs_fused_hip.h) are pinned symbol by symbol, so this entry has a header of its own.  Same library, same
 * conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_* return
 * codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_PVOS_HIP_H
#define UNIVS_PVOS_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scoring a VIPOSeg panoptic-VOS result (csrc/pvos_count.hip) ------------------------------------------------------------------------
 * gt / pred: uint8 [T, H, W], the id maps of the annotation and the result PNGs of one video.  counts: int32 [T, K, 6], ZEROED BY THE
 * CALLER; cell [t, k - 1] = (I, A_g, A_p, BI, B_g, B_p) of id k in frame t: the pixels with gt == pred == k, gt == k, pred == k, and the
 * same three among boundary pixels (BI: gt == pred == k and boundary on both sides).  A pixel is a boundary pixel of its own id in a map
 * exactly when the (2 d + 1) x (2 d + 1) window around it holds another label of that map or leaves the image: what
 * mask - erode(copyMakeBorder(mask, 1 pixel of 0), 3 x 3 ones, iterations = d) leaves of every id's mask.  Ids 0 and above K are not
 * counted; as labels they still break a window's uniformity.
 * d <= 88 (a 4K frame's round(0.02 diagonal)), K <= 255 and T H W < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED.  T, H, W, d or K < 1 is an
 * invalid argument.
 * Replaces: the two `mask_to_boundary` calls and the mask sums per (tracked object, frame) of `eval_iou`
 * (univs/evaluation/pvos_evaluation.py:185-201, eval_utils_viposeg.py:27-80). */
int univs_pvos_counts(const uint8_t* gt, const uint8_t* pred, int T, int H, int W, int d, int K, int32_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_PVOS_HIP_H */
