/* libunivs_hip.so, seventeenth header: the labels of a per-image semantic result without its [C, H, W] tensor, and the confusion matrix
 * of two label maps.  The sixteen other headers are pinned symbol by symbol, so these two entries have a header of their own.  Same
 * library, same conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the
 * UNIVS_* return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_IMAGELABELS_HIP_H
#define UNIVS_IMAGELABELS_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- labels[y, x] = argmax_c bilinear(r_c -> H x W)(y, x) (csrc/semseg_labels.hip) ---------------------------------------------------------
 * r: float32 [C, hi, wi]; labels: uint8 [H, W], written in full.  The resize is univs_bilinear_resample_f32's (align_corners = false,
 * ATen's source index, the same taps, weights and roundings: every compared value carries the bits that call would have stored); the
 * first maximum wins, i.e. strict > while c ascends, which is ATen's argmax on finite inputs.  The order of NaNs is not specified.
 * One pass over r; the [C, H, W] tensor is never built.
 * C, hi, wi, H or W < 1 is an invalid argument.
 * Covered: C <= 256, H W < 2^31, hi wi < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: `sem_seg_postprocess` (F.interpolate(r, size, mode="bilinear", align_corners=False)) followed by the `argmax(dim=0)` of
 * detectron2's SemSegEvaluator.process. */
int univs_semseg_labels_f32(const float* r, int C, int hi, int wi, int H, int W, uint8_t* labels, void* stream);

/* ---- conf[row, col] += 1 per pixel of two label maps (csrc/semseg_labels.hip) -----------------------------------------------------------------
 * gt, pred: uint8 [n].  conf: int64 [(K + 1), (K + 1)], K = num_classes, which the call ADDS to: row = the ground truth with
 * ignore_label -> K, column = the prediction (0 .. K).  stray: int64 [2], added to as well: stray[0] = the pixels whose ground truth is
 * neither < K nor ignore_label, stray[1] = those whose prediction is > K.  A stray pixel is counted there and nowhere else; it never
 * indexes the matrix.  ignore_label = -1: no value is ignored.
 * n < 0, num_classes < 1, or an ignore_label outside {-1} and [num_classes, 255] is an invalid argument; n == 0 is success and launches
 * nothing.
 * Covered: (K + 1)^2 <= 32768 cells (a workgroup's int32 histogram in 128 KB of LDS), n < 2^31 - 4, gt and pred aligned to 4 bytes, conf
 * and stray to 8; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.  The maps' last dword is read whole: up to three bytes
 * past n, which an allocation's rounding holds.
 * Replaces: `np.bincount((K + 1) * pred + gt, minlength=(K + 1)^2)` of detectron2's SemSegEvaluator.process (transposed: here the row
 * is the ground truth, the orientation univs_amd/evaluation/vss.py reads). */
int univs_label_confusion_u8(const uint8_t* gt, const uint8_t* pred, long long n, int num_classes, int ignore_label, long long* conf,
                             long long* stray, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_IMAGELABELS_HIP_H */
