/* libunivs_hip.so, nineteenth header: polygon segmentations (COCO's instance ground truth) to the run-length boundaries the overlap
 * kernels read.  The eighteen other headers are pinned symbol by symbol, so this entry has a header of its own.  Same library, same
 * conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_* return
 * codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_POLYGONS_HIP_H
#define UNIVS_POLYGONS_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- all objects of a call, each a list of polygons, to cumulative column-major run boundaries (csrc/polygon_runs.hip) ------------------
 * The rule is univs_amd/data/polygon_rule.py: vertices scaled by 5, the points along every edge, a crossing wherever two successive
 * points lie on two sides of a pixel column's centre line, the crossings' parity per polygon, the union of an object's polygons.
 * xy: float64 [2 n_points], x0 y0 x1 y1 ... of all polygons back to back.  poly_start: int32 [P + 1], polygon p owns the points
 * poly_start[p] .. poly_start[p + 1].  obj_start: int32 [N + 1], object o owns the polygons obj_start[o] .. obj_start[o + 1] (none: the
 * object is absent).  size: int32 [N, 2], the h and w of every object's image.  slot: int64 [N + 1], object o may write
 * bounds / ones [slot[o], slot[o + 1]); cap_total: the length of both.  All ON THE DEVICE.
 * Written per object: count[o] boundaries (0 for an absent object, else the ascending boundaries of the union's runs, odd runs
 * foreground, the first one possibly 0, the last one h w) and as many `ones` (the foreground pixels before the boundary) into its
 * slots, and status[o]:
 *   0 done   1 more than 16384 crossings   2 a polygon of more than 2^22 points   3 h < 1, w < 1 or h w >= 2^31
 *   4 a polygon of more than 4096 vertices   5 a polygon of fewer than 3 points, or a coordinate that is not finite or beyond +-2^24
 *   6 fewer slots than boundaries
 * With a status other than 0 the count is 0 and the caller rasterises that object elsewhere (1 to 4) or refuses it (5, 6).
 * The kernel trusts no entry of the four tables: each is clamped into its array before it indexes anything, every loop is counted by a
 * clamped number, every store is checked against the object's own slots.
 * N < 0, P < 0, n_points < 0 or cap_total < 0 is an invalid argument; N == 0 is success and launches nothing.
 * Covered: n_points < 2^31 and cap_total < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched. */
int univs_polygons_to_runs(const double* xy, const int* poly_start, const int* obj_start, const int* size, const long long* slot,
                           long long n_points, int P, int N, long long cap_total, int* bounds, int* ones, int* count, int* status,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_POLYGONS_HIP_H */
