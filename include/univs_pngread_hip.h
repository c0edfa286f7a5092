/* libunivs_hip.so, twelfth header: label PNGs read on the device.  The host parses the container and uploads the zlib streams; the
 * device inflates them, undoes the row filters and writes the planes the count kernels take.  The eleven other headers are pinned
 * symbol by symbol, so this entry has a header of its own.  Same library, same conventions: plain pointers and sizes, device pointers,
 * `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_* return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_PNGREAD_HIP_H
#define UNIVS_PNGREAD_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- N PNG images from their zlib streams (csrc/png_inflate.hip, csrc/png_inflate_core.h) ----------------------------------------------------
 * streams: the concatenated IDAT payloads of the N files back to back, streams_total bytes; stream_offsets: int64 [N + 1], file f is
 * streams[stream_offsets[f] : stream_offsets[f + 1]].  desc: int32 [N, 8] = W, H, colour type, bit depth, out channels, palette row, 0, 0
 * from the file's IHDR.  palettes: uint8 [P, 256, 3], a file's PLTE padded with zeros (a missing entry is black), or NULL with P == 0.
 * filtered: scratch of filt_total bytes; file f's H (1 + rowbytes) inflated bytes (RFC 1950 / 1951; rowbytes = ceil(W bits per pixel
 * / 8)) start at filtered[filt_offsets[f]] and are kept.  out: out_total bytes; file f's plane starts at out[out_offsets[f]]:
 *   out channels 1   [H, W]     the palette indices (1 / 2 / 4-bit rows unpacked, MSB first) or the grey values
 *   out channels 3   [H, W, 3]  RGB as stored, grey replicated, or palette row `palette row` looked up
 * which is `np.array(PIL.Image.open(f))` and `np.array(PIL.Image.open(f).convert("RGB"))`.  A file's regions
 * [filt_offsets[f], filt_offsets[f + 1]) and [out_offsets[f], out_offsets[f + 1]) may be larger than it needs: the rest is not
 * touched.  No byte outside a file's own regions is read or written, whatever its stream holds.
 * status: int32 [N], per file 0 or the first rule its bytes broke; the plane of a file with a non-zero status is unspecified:
 *    1  descriptor or offsets: W or H < 1, a colour type / bit depth / out channels outside the coverage, palette row outside [0, P),
 *       rowbytes > max_rowbytes, a region outside its buffer or smaller than the file needs
 *    2  zlib header (CM != 8, window > 32 KB, FCHECK, preset dictionary)     3  input exhausted
 *    4  block type 3              5  LEN != ~NLEN of a stored block           6  over-subscribed or forbidden incomplete code,
 *    7  repeat code with no previous length or past the block's lengths          HLIT > 286, HDIST > 30, no end-of-block code
 *    8  literal/length symbol 286 / 287, distance code 30 / 31, bits that are no code
 *    9  distance beyond the bytes produced     10  more than H (1 + rowbytes) bytes     11  fewer, at the end of the final block
 *   12  Adler-32                               13  a filter byte above 4
 * N, P or a total < 0, max_rowbytes < 1, or P > 0 with NULL palettes is an invalid argument; N == 0 is success and launches nothing.
 * Covered: W, H >= 1; colour type 0 or 2 at bit depth 8, colour type 3 at bit depth 1, 2, 4 or 8; non-interlaced; max_rowbytes (the
 * caller's bound on every file's rowbytes) <= 24576, which admits 8191 RGB pixels per row, the encoder's own cap; streams_total,
 * filt_total and out_total < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: `PIL.Image.open` + `np.array` per file on one host core and the upload of the decoded planes in the file scorers
 * (evaluation/vps.py, vss.py, davis.py, pvos.py). */
int univs_png_read(const uint8_t* streams, const long long* stream_offsets, const int* desc, const uint8_t* palettes, int P,
                   const long long* filt_offsets, const long long* out_offsets, int N, long long streams_total, long long filt_total,
                   long long out_total, int max_rowbytes, uint8_t* filtered, uint8_t* out, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_PNGREAD_HIP_H */
