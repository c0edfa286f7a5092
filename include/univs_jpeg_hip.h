/* libunivs_hip.so, thirteenth header: baseline JPEG frames decoded on the device.  The host walks the marker segments and uploads the
 * tables and the entropy-coded bytes; the device removes the byte stuffing, decodes the Huffman data in parallel, runs the inverse DCT
 * and writes RGB frames.  The twelve other headers are pinned symbol by symbol, so this entry has a header of its own.  Same library,
 * same conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_*
 * return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_JPEG_HIP_H
#define UNIVS_JPEG_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- N JPEG files of one size and sampling (csrc/jpeg_decode.hip, csrc/jpeg_entropy_core.h) -----------------------------------------------
 * src: the files' bytes from the end of the SOS header to the end of the file, back to back, src_total bytes; src_off: int64 [N + 1].
 * ri: int32 [N], the restart interval in MCUs (0: none).  huff: uint8 [N, 6, 272], row 2 c the DC and row 2 c + 1 the AC table of
 * component c as in a DHT segment, 16 counts and the values padded to 256 (ncomp == 1: rows 0 and 1).  quant: uint16 [N, 3, 64],
 * component c's table in natural (row-major) order.  W, H: the frame; ncomp 1 (grey, h = v = 1) or 3 (Y Cb Cr, luma sampled h x v,
 * chroma 1 x 1).  subseq_bits: bits of a subsequence of the parallel entropy decode, a multiple of 32.  max_intervals: at least
 * ceil(MCUs / ri) of every file.  phases: 1 the entropy launches (status, rounds and blocks are cleared first), 2 the pixel launches
 * (on the blocks and status that are there), 3 both.
 * Scratch: comp, src_total bytes (the data without stuffing); ivl, int32 [N, max_intervals + 1] (interval starts); blocks, int16
 * [N, MCUs blocks-per-MCU, 64], the coefficients in scan order, natural order inside a block, DC absolute, kept; planes, uint8
 * [N, plane bytes], 8-byte aligned: each component padded to whole MCUs.
 * out: uint8 [N, H, W, 3], 4-byte aligned: np.asarray(PIL.Image.open(f).convert("RGB")) of every file whose status is 0 (Pillow on
 * libjpeg-turbo with its defaults: islow IDCT, fancy upsampling); the pixels of any other file are unspecified.  No byte outside a file's
 * own regions is read or written, whatever its data holds.
 * status: int32 [N], per file 0 or the OR of
 *     1  an offset or the restart interval not admissible             2  a Huffman table with an over-subscribed length
 *     4  bits that are no code              8  a zero run past the end of a block         16  data exhausted before the blocks
 *    32  restart markers out of sequence, or not as many intervals as ri and the frame give
 *    64  a magnitude category above 11 (DC) / 10 (AC)                128  a DC value outside int16
 *   256  outside the range in which the rule is pinned: |coef q| > 32767, a first-pass IDCT output outside int16 or a second-pass
 *        value outside [-512, 511]                                   512  the data is not ended by an EOI marker
 * rounds: int32 [N], the most synchronisation rounds a chunk of the file took.
 * N < 0, src_total < 0, max_intervals < 1 or phases outside 1..3 is an invalid argument; N == 0 is success and launches nothing.
 * Covered: 16 <= W, H <= 16384; (ncomp, h, v) in {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}; 32 <= subseq_bits <= 2^20, a multiple
 * of 32; max_intervals <= 2^20; src_total and 3 N H W < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: `PIL.Image.open(f).convert("RGB")` per frame on one host core and the upload of the decoded frames in the test mappers
 * (data/mapper.py). */
int univs_jpeg_decode(const uint8_t* src, const long long* src_off, const int* ri, const uint8_t* huff, const uint16_t* quant, int N, int W,
                      int H, int ncomp, int h, int v, int subseq_bits, int max_intervals, long long src_total, int phases, uint8_t* comp,
                      int* ivl, int16_t* blocks, uint8_t* planes, uint8_t* out, int* status, int* rounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_JPEG_HIP_H */
