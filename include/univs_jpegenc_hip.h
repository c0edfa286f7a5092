/* libunivs_hip.so, fourteenth header: baseline JPEG files encoded on the device, optionally with a result overlaid on the frames.  The
 * device converts the colours, runs the forward DCT, quantises, Huffman-codes and stuffs the bytes; the host writes the marker segments
 * around them.  The thirteen other headers are pinned symbol by symbol, so this entry has a header of its own.  Same library, same
 * conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_* return
 * codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_JPEGENC_HIP_H
#define UNIVS_JPEGENC_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- N frames of one size to the entropy-coded data of N JPEG files (csrc/jpeg_encode.hip) ------------------------------------------------
 * rgb: uint8 [N, H, W, 3].  ids: NULL, or the result to overlay, [N, H, W] uint8 (ids_is_i32 == 0) or int32 (ids_is_i32 == 1), with lut:
 * uint8 [K, 4] = (r, g, b, alpha) and edge: -1 or the contour colour 0xRRGGBB.  Per pixel k = min(max(id, 0), K - 1), a = lut[k][3],
 * out_c = (rgb_c (255 - a) + lut[k][c] a + 127) / 255; where edge >= 0, a > 0 and a 4-neighbour inside the image has another k, the pixel
 * is the contour colour.  No overlaid frame is stored.  Without ids, lut, K and edge are not looked at.
 * h, v: the sampling of the luma, (1, 1) 4:4:4, (2, 1) 4:2:2, (2, 2) 4:2:0; chroma is 1 x 1.  quality: libjpeg's, 1..100.
 * The data of frame i is that of `PIL.Image.fromarray(frame).save(f, "JPEG", quality=quality, subsampling=s)` (Pillow on libjpeg-turbo
 * with its defaults: islow DCT, the Annex K tables, one interleaved scan, no restart intervals) byte for byte, from after the SOS header
 * to before the EOI marker.
 * phases: 1 the coefficient launches: status is cleared; blocks, int16 [N, B, 64], 16-byte aligned, B = MCUs x (h v + 2): the quantised
 * coefficients in scan order, zig-zag order inside a block, DC absolute, dummy blocks included; sizes, uint32 [N, B]: the bits of every
 * block; bit_off, int64 [N, B]: their exclusive sum; totals, int64 [N]: the bits of every frame.  2 the stream launches, on what phase 1
 * left: raw_off, int64 [N + 1], multiples of 4, frame i's region raw_off[i] .. raw_off[i + 1] at least ceil(totals[i] / 8) rounded up
 * to 4; raw, raw_total >= raw_off[N] bytes, 4-byte aligned, scratch (the data before stuffing); out, 2 raw_total bytes: frame i's data
 * from 2 raw_off[i]; out_len, int64 [N], its length.  3 both.  With phases == 1 raw_off, raw, out and out_len may be NULL.
 * status: int32 [N], per frame 0 or the OR of
 *     1  a DC difference of a category above 11        2  an AC coefficient of a category above 10 (neither is reachable from 8-bit
 *     samples as far as known)                         4  the frame's region of raw is not admissible or too small: nothing was written
 * N < 0, phases outside 1..3, raw_total < 0, ids with K < 1 or edge outside -1..0xFFFFFF is an invalid argument; N == 0 is success and
 * launches nothing.  Covered: 1 <= W, H <= 16384; (h, v) in {(1, 1), (2, 1), (2, 2)}; 1 <= quality <= 100; 3 N H W < 2^31;
 * raw_total < 2^40; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: the overlay drawn on the host and `PIL.Image.save` per frame on one host core, and the download of the frames. */
int univs_jpeg_encode(const uint8_t* rgb, const void* ids, int ids_is_i32, const uint8_t* lut, int K, int edge, int N, int H, int W, int h,
                      int v, int quality, int phases, int16_t* blocks, uint32_t* sizes, long long* bit_off, long long* totals,
                      const long long* raw_off, long long raw_total, uint8_t* raw, uint8_t* out, long long* out_len, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_JPEGENC_HIP_H */
