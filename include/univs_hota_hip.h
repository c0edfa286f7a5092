/* libunivs_hip.so, eleventh header: the HOTA tables of one video from its overlap table, and the batched assignment solver behind
 * them.  The ten other headers are pinned symbol by symbol, so these entries have a header of their own.  Same library, same
 * conventions: plain pointers and sizes, device pointers, `stream` (a hipStream_t, NULL = the default stream) last, the UNIVS_*
 * return codes and univs_last_error() of univs_hip.h. */
#ifndef UNIVS_HOTA_HIP_H
#define UNIVS_HOTA_HIP_H

#include <stdint.h>

#include "univs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- what HOTA counts in one video, for all of its class sequences in one launch (csrc/hota_count.hip) ------------------------------------
 * inter: int32 [D, G, T], the per-frame overlap of result track d and ground-truth track g exactly as univs_vis_overlap_counts wrote
 * it.  gt_area: int32 [G, T], tr_area: int32 [D, T], the per-frame areas; 0 = the id is absent from the frame.  Class c owns the ground
 * truths gt_ids[gt_starts[c] : gt_starts[c + 1]] (indices into G) and the tracks tr_ids[tr_starts[c] : tr_starts[c + 1]] (indices into
 * D); gt_starts and tr_starts are int32 [C + 1], ascending from 0.  max_g / max_p: the largest number of ids a class has on either
 * side (the CALLER's statement of what the device lists hold; a class that exceeds 64 all the same is skipped, its outputs untouched).
 * An id outside its table is clamped: it costs a wrong number, never an address outside the inputs.  thresholds: float64 [A], already
 * alpha - eps.
 * Outputs, per class, packed by the same starts; the caller fills match_col with -1 and the others with 0 before the call:
 *   tp_fn_fp int32 [C, A, 3]; matches int32 [A, g, p] of class c at A sum_{c' < c} g' p'; loca_sum float64 [C, A]; gt_id_count int32 at
 *   gt_starts[c]; tracker_id_count int32 at tr_starts[c]; match_col int32 [T, g] of class c at T gt_starts[c]: the class-local track
 *   assigned to the ground truth in that frame where their similarity is above 0, else -1.
 * The rule is univs_amd/evaluation/hota_counts.py's (hota_counts_aten): similarity I / (A_g + A_p - I) in float64, the global alignment
 * pass, one linear assignment per frame maximising sum gas similarity, the tally at every threshold in frame order.  Where a frame's
 * optimum is unique the tables are the rule's, loca_sum bit for bit; among equal totals the solver's tie rule decides (an unassigned
 * column first, then the lowest index).
 * D, G, T, C or A < 1, max_g or max_p < 0 is an invalid argument.
 * Covered: max_g <= 64, max_p <= 64, A <= 32, T <= 65535, D G T < 2^31; else UNIVS_ERR_NOT_IMPLEMENTED, before anything is launched.
 * Replaces: the three Python frame loops of TrackEval's HOTA.eval_sequence with one scipy linear_sum_assignment call per frame. */
int univs_hota_counts(const int32_t* inter, const int32_t* gt_area, const int32_t* tr_area, int D, int G, int T, const int32_t* gt_ids,
                      const int32_t* gt_starts, const int32_t* tr_ids, const int32_t* tr_starts, int C, int max_g, int max_p,
                      const double* thresholds, int A, int32_t* tp_fn_fp, int32_t* matches, double* loca_sum, int32_t* gt_id_count,
                      int32_t* tracker_id_count, int32_t* match_col, void* stream);

/* ---- the solver alone: B small assignment problems, one wave each (csrc/hota_count.hip) ----------------------------------------------------
 * score: float64 [B, 64, 64] (row pitch 64 whatever the problem's size); problem b is the top-left rows[b] x cols[b] corner and is
 * MAXIMISED: every row of the smaller side gets a distinct column / row of the larger.  rows, cols: int32 [B], each in 1..64; a
 * problem outside that is skipped.  col_of_row: int32 [B, 64]: the column of row r < rows[b], -1 for the rows left over when
 * rows[b] > cols[b]; entries from rows[b] on are not written.  Scores have to be finite.
 * Shortest augmenting paths in float64 with counted loops; among equal distances an unassigned column first, then the lowest index.
 * B < 0 is an invalid argument; B == 0 is success and launches nothing. */
int univs_lsa_max_f64(const double* score, const int32_t* rows, const int32_t* cols, int B, int32_t* col_of_row, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNIVS_HOTA_HIP_H */
