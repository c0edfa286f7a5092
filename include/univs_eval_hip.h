/* libunivs_hip.so, second header: entries of the evaluation that were added after include/univs_hip.h was pinned symbol by symbol
 * (tests/capi_signatures.txt).  Same library, same conventions: plain pointers and sizes, device pointers unless stated, `stream` (a
 * hipStream_t, NULL = the default stream) last, the UNIVS_* return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_EVAL_HIP_H
#define UNIVS_EVAL_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scoring a YouTube-VIS result (csrc/vis_overlap.hip) --------------------------------------------------------------------------------
 * The per-frame overlaps of every detection and every ground truth of one video, read off the run-length codes; no mask is decoded.
 * Both sides in one layout: `bounds` int32, the cumulative column-major run boundaries of all masks back to back; mask m owns
 * bounds[starts[m] : starts[m + 1]], its run k covers [b_{k-1}, b_k) with b_{-1} = 0, odd runs are foreground, the last boundary is H W.
 * gt_ones[k]: the foreground pixels of the mask in [0, b_k).  starts int32 [masks + 1]; starts[m + 1] == starts[m] is an absent (None)
 * mask, which counts as an empty one.  Detection masks are d T + t, ground-truth masks g T + t.
 * gt_max_bounds: the largest boundary count of a ground-truth mask (the LDS tile of the launch); a mask with more stores -1 in its cells.
 * inter [D, G, T] int32: |d_t AND g_t|; every cell is written exactly once, the caller need not zero it.
 * H W < 2^31, T <= 65535 and gt_max_bounds <= 16384 (128 KB of LDS); else UNIVS_ERR_NOT_IMPLEMENTED.  D G T >= 2^31 is an invalid argument.
 * Replaces: YTVOSeval.computeIoU's maskUtils.merge / maskUtils.area calls per (detection, ground truth, frame)
 * (univs/data/datasets/ytvis_api/ytvoseval.py:173-219): iou_seq = I / (A_d + A_g - I), I the sum of inter over t, A the summed areas. */
int univs_vis_overlap_counts(const int32_t* dt_bounds, const int32_t* dt_starts, const int32_t* gt_bounds, const int32_t* gt_ones,
                             const int32_t* gt_starts, int D, int G, int T, int H, int W, int gt_max_bounds, int32_t* inter, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_EVAL_HIP_H */
