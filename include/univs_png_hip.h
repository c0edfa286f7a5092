/* libunivs_hip.so, tenth header: the zlib streams of result PNGs, encoded on the device from the id maps.  The nine other headers are
 * pinned symbol by symbol, so this entry has a header of its own.  Same library, same conventions: plain pointers and sizes, device
 * pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_* return codes and univs_last_error() of
 * univs_hip.h. */
#ifndef UNIVS_PNG_HIP_H
#define UNIVS_PNG_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one zlib stream per frame of a stack of id maps (csrc/png_deflate.hip) ----------------------------------------------------------------
 * src: the id maps [N, H, W] on the device, uint8 (src_is_i32 == 0) or int32.  lut: uint8 [K, C] on the device, C in {1, 3}: the pixel
 * bytes are lut[clamp(id, 0, K - 1)], so the colours of a panoptic map or the class remap of a semantic map are applied inside the
 * encoder and no pixel plane exists; a NULL lut is the identity and needs uint8 ids and C == 1.  A bad id is clamped: it costs a wrong
 * pixel, never an address outside the inputs.
 * The format is the one of univs_amd/inference/png_rule.py, byte for byte (tests/test_png_deflate_gpu.py): the rows filtered with "None",
 * runs at distance C and literals in RFC 1951's fixed Huffman code, one deflate block and an empty stored block per stripe of
 * rows_per_stripe rows, 78 01 before, 03 00 and the Adler-32 after.  rows_per_stripe is part of the format and the CALLER's to supply:
 * it has to be png_rule.stripe_rows(W C + 1), or the streams, still valid, are not the rule's.
 * out: the N streams back to back; offsets: int64 [N + 1] on the device, stream f is out[offsets[f] : offsets[f + 1]].  With
 * S = ceil(H / rows_per_stripe) and cap = ceil((9 rows_per_stripe (W C + 1) + 13) / 8) + 4 (png_rule.stripe_capacity), `out` needs
 * N (8 + S cap) bytes and `scratch` N S (16 + cap) bytes (png_rule.scratch_bytes); scratch is 4-byte aligned.
 * N < 0, H, W, C or rows_per_stripe < 1, K < 1 with a lut, or a NULL lut with int32 ids or C != 1 is an invalid argument; N == 0 is
 * success and launches nothing.
 * Covered: C in {1, 3}, rows_per_stripe (W C + 1) <= 24576 (the stripe's bytes in LDS), N H (W C + 1) < 2^31; else
 * UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: the download of the planes and `PIL.Image.save` per frame (zlib level 6 on one host core) in save_vos_results,
 * VPSEvaluator.process and VSSEvaluator.process.  Pinned to zlib's and Pillow's decoders, not to their encoders: the files differ
 * from Pillow's and are larger. */
int univs_png_deflate_maps(const void* src, int src_is_i32, int N, int H, int W, const uint8_t* lut, int K, int C, int rows_per_stripe,
                           uint8_t* scratch, uint8_t* out, long long* offsets, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_PNG_HIP_H */
