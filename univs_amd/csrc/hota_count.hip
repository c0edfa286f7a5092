// What HOTA (TrackEval's metric, univs/evaluation/eval_hota.py:25-117 in the reference) does with the overlap table of one video, for
// every class sequence at once (univs_amd/evaluation/hota_counts.py states the rule in numpy, hota.py the protocol around it).  The
// reference walks the frames three times in Python and calls scipy.optimize.linear_sum_assignment once per frame.
//
// inter: int32 [D, G, T] as vis_overlap.hip wrote it (D result tracks, G ground-truth tracks of the video).  gt_area [G, T], tr_area
// [D, T]: int32, 0 = the id is absent from the frame.  Class c owns the ground truths gt_ids[gt_starts[c] : gt_starts[c + 1]] (indices
// into G) and the tracks tr_ids[tr_starts[c] : tr_starts[c + 1]] (indices into D); g and p below are its two counts.  thr: float64
// [A], already alpha - eps.  Outputs, packed by the same starts; the caller fills match_col with -1 and the others with 0:
//   tp_fn_fp [C, A, 3]  matches [A, g, p] at A sum_{c' < c} g' p'  loca_sum [C, A]  gt_id_count at gt_starts[c]  tracker_id_count at
//   tr_starts[c]  match_col [T, g] at T gt_starts[c]: the class-local track matched to the ground truth in that frame with a
//   similarity above 0, else -1
//
// One workgroup of 256 threads per class, three phases:
//  1 alignment   frame by frame: the areas of the class to LDS, the row and column sums of the similarities (one lane per id, ascending
//                partner), then every (g, p) cell, owned by one lane for the whole walk, adds sim / (colsum + rowsum - sim) to its
//                float64 cell of LDS, guarded as in the reference.  Then gas = cell / (count_g + count_p - cell) where both ids occur;
//                the other cells are never read.
//  2 assignment  one wave per frame, frames strided over the four waves: maximise sum gas sim over the present ids by shortest
//                augmenting paths (Jonker-Volgenant without initialisation, lsa_wave below).
//  3 tally       lane a of wave 0 owns threshold a and walks the frames ascending, the matched pairs of a frame in ascending
//                ground-truth row; the frame's partial sum starts from 0 and is added to loca_sum[a], as Python's sum() and += do.
// similarity = (double)I / (double)(A_g + A_p - I): one IEEE division.  This file is compiled with -ffp-contract=off (build.py), so
// the products and sums below stay separate operations in the order written.
//
// LDS: gas 64 x 64 float64 (32 KB), per wave the frame's overlaps 64 x 64 int32 (16 KB) and four 64-entry lists; 100.6 KB in all, one
// workgroup per CU.  A video has few classes, so the grid is small whatever the occupancy; nothing here is tuned or measured.
#include "count_core.h"
#include "launchers.h"

namespace univs {

constexpr int HO_N = 64;                                          // ids per side of a class sequence: lanes of a wave
constexpr int HO_A_MAX = 32;
constexpr int HO_WAVES = 4;
#define HO_INF (__builtin_huge_val())

// argmin over the wave of (val, key), val first, then the smaller key; every lane gets the winner
__device__ __forceinline__ void wave_argmin(double& val, int& key) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const double ov = __shfl_xor(val, m, 64);
    const int ok = __shfl_xor(key, m, 64);
    if (ov < val || (ov == val && ok < key)) {
      val = ov;
      key = ok;
    }
  }
}

// Linear assignment of nr rows to nc columns (1 <= nr <= nc <= 64) minimising sum cost(i, j), by one wave: lane j is column j.
// cost(i, j) is called by lane j for the wave-uniform row i.  Returns, in lane i < nr, the column of row i (row4col: in lane j < nc the
// row of column j, or -1).  Shortest augmenting paths as scipy.optimize.linear_sum_assignment documents them (Crouse 2016), duals and
// distances in float64.  The column with the least distance is a wave reduction; among equal distances an unassigned column wins, then
// the lowest index: the first half is SciPy's rule, the second this project's.  Every loop is counted: nr augmentations, at most nc
// selections each (a selection retires a column, and nr <= nc leaves an unassigned one to end on), at most nr steps back along a path;
// no exit waits for a floating-point comparison.
template <typename Cost>
__device__ __forceinline__ int lsa_wave(int nr, int nc, int lane, Cost cost, int& row4col) {
  double u = 0.0, v = 0.0;                                         // u: lane as row, v: lane as column
  int col4row = -1;                                                // lane as row
  row4col = -1;
  for (int cur = 0; cur < nr; ++cur) {
    double spc = HO_INF, min_val = 0.0;
    int path = -1, i = cur, sink = -1;
    bool in_sc = false, in_sr = false;
    for (int step = 0; step < nc && sink < 0; ++step) {
      if (lane == i) in_sr = true;
      const double ui = __shfl(u, i, 64);
      const bool open = lane < nc && !in_sc;
      if (open) {
        const double r = min_val + cost(i, lane) - ui - v;
        if (r < spc) {
          spc = r;
          path = i;
        }
      }
      double val = open ? spc : HO_INF;
      int key = open ? ((row4col >= 0 ? 256 : 0) | lane) : 0x7fff;
      wave_argmin(val, key);
      key = __builtin_amdgcn_readfirstlane(key);
      val = __shfl(val, 0, 64);
      int j = key & 255;
      if (key == 0x7fff) j = __ffsll((long long)__ballot(open)) - 1;   // (only if a distance is not a number: keep counting down)
      if (j < 0) break;
      min_val = val;
      const int r4 = __shfl(row4col, j, 64);
      if (lane == j) in_sc = true;
      if (r4 < 0) sink = j; else i = r4;
    }
    if (sink < 0) break;                                           // (unreachable for finite costs)
    const double spc_mine = __shfl(spc, col4row >= 0 ? col4row : 0, 64);
    if (lane == cur) u += min_val;
    else if (in_sr) u += min_val - spc_mine;
    if (in_sc) v -= min_val - spc;
    int j = sink;
    for (int k = 0; k < nr; ++k) {
      const int i2 = __shfl(path, j, 64);
      if (i2 < 0) break;
      if (lane == j) row4col = i2;
      const int prev = __shfl(col4row, i2, 64);
      if (lane == i2) col4row = j;
      j = prev;
      if (i2 == cur || j < 0) break;
    }
  }
  return col4row;
}

__device__ __forceinline__ double ho_sim(int inter, int ag, int ap) { return (double)inter / (double)((long long)ag + ap - inter); }

// the carve-up of the dynamic LDS, in bytes
constexpr int HO_LDS_GAS = 0;                                      // double [64][64]
constexpr int HO_LDS_ROW = HO_LDS_GAS + HO_N * HO_N * 8;           // double [64] row sums, double [64] column sums
constexpr int HO_LDS_IDS = HO_LDS_ROW + 2 * HO_N * 8;              // int [64] gt ids, [64] track ids, [64] gt areas, [64] track areas, [64] + [64] counts
constexpr int HO_LDS_WAVE = HO_LDS_IDS + 6 * HO_N * 4;             // per wave: int [64][64] overlaps, int [4][64] lists
constexpr int HO_LDS_PER_WAVE = HO_N * HO_N * 4 + 4 * HO_N * 4;
constexpr int HO_LDS_TOTAL = HO_LDS_WAVE + HO_WAVES * HO_LDS_PER_WAVE;

__global__ __launch_bounds__(256) void hota_count_kernel(const int* __restrict__ inter, const int* __restrict__ gt_area,
                                                         const int* __restrict__ tr_area, int D, int G, int T,
                                                         const int* __restrict__ gt_ids, const int* __restrict__ gt_starts,
                                                         const int* __restrict__ tr_ids, const int* __restrict__ tr_starts,
                                                         const double* __restrict__ thr, int A, int* __restrict__ tp_fn_fp,
                                                         int* __restrict__ matches, double* __restrict__ loca_sum,
                                                         int* __restrict__ gt_id_count, int* __restrict__ tracker_id_count,
                                                         int* __restrict__ match_col) {
  extern __shared__ __align__(8) unsigned char ho_lds[];
  double* gas = reinterpret_cast<double*>(ho_lds + HO_LDS_GAS);
  double* rowsum = reinterpret_cast<double*>(ho_lds + HO_LDS_ROW);
  double* colsum = rowsum + HO_N;
  int* gid = reinterpret_cast<int*>(ho_lds + HO_LDS_IDS);
  int* pid = gid + HO_N;
  int* s_ag = pid + HO_N;
  int* s_ap = s_ag + HO_N;
  int* s_gc = s_ap + HO_N;
  int* s_pc = s_gc + HO_N;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = blockIdx.x;
  const int g0 = gt_starts[c], p0 = tr_starts[c];
  const int g = gt_starts[c + 1] - g0, p = tr_starts[c + 1] - p0;
  if (g < 0 || p < 0 || g > HO_N || p > HO_N || g0 < 0 || p0 < 0) return;      // (the whole workgroup; the entry has refused such a call)
  long long mo = 0;
  for (int k = 0; k < c; ++k) mo += (long long)(gt_starts[k + 1] - gt_starts[k]) * (tr_starts[k + 1] - tr_starts[k]);
  int* my_matches = matches + mo * A;
  int* my_match_col = match_col + (long long)T * g0;

  // the ids of the class, clamped: a bad id costs a wrong number, never an address outside the tables
  if (tid < g) gid[tid] = min(max(gt_ids[g0 + tid], 0), G - 1);
  if (tid >= 64 && tid - 64 < p) pid[tid - 64] = min(max(tr_ids[p0 + tid - 64], 0), D - 1);
  for (int i = tid; i < HO_N * HO_N; i += 256) gas[i] = 0.0;
  __syncthreads();

  // ---- 1: alignment ------------------------------------------------------------------------------------------------------------------
  const double eps = 2.220446049250313e-16;                        // np.finfo('float').eps
  int present = 0;                                                 // thread gl < g: frames with the ground truth; 64 + pl: with the track
  for (int t = 0; t < T; ++t) {
    if (tid < g) {
      const int a = gt_area[(long long)gid[tid] * T + t];
      s_ag[tid] = a;
      present += a > 0;
    } else if (tid >= 64 && tid - 64 < p) {
      const int a = tr_area[(long long)pid[tid - 64] * T + t];
      s_ap[tid - 64] = a;
      present += a > 0;
    }
    __syncthreads();
    if (tid < g) {
      double s = 0.0;
      const int ag = s_ag[tid];
      if (ag > 0)
        for (int pl = 0; pl < p; ++pl)
          if (s_ap[pl] > 0) s += ho_sim(inter[((long long)pid[pl] * G + gid[tid]) * T + t], ag, s_ap[pl]);
      rowsum[tid] = s;
    } else if (tid >= 64 && tid - 64 < p) {
      double s = 0.0;
      const int ap = s_ap[tid - 64];
      if (ap > 0)
        for (int gl = 0; gl < g; ++gl)
          if (s_ag[gl] > 0) s += ho_sim(inter[((long long)pid[tid - 64] * G + gid[gl]) * T + t], s_ag[gl], ap);
      colsum[tid - 64] = s;
    }
    __syncthreads();
    for (int cell = tid; cell < g * p; cell += 256) {
      const int gl = cell / p, pl = cell - gl * p;
      const int ag = s_ag[gl], ap = s_ap[pl];
      if (ag > 0 && ap > 0) {
        const double sim = ho_sim(inter[((long long)pid[pl] * G + gid[gl]) * T + t], ag, ap);
        const double denom = colsum[pl] + rowsum[gl] - sim;
        if (denom > 0.0 + eps) gas[gl * HO_N + pl] += sim / denom;
      }
    }
    __syncthreads();
  }
  if (tid < g) {
    s_gc[tid] = present;
    gt_id_count[g0 + tid] = present;
  } else if (tid >= 64 && tid - 64 < p) {
    s_pc[tid - 64] = present;
    tracker_id_count[p0 + tid - 64] = present;
  }
  __syncthreads();
  for (int cell = tid; cell < g * p; cell += 256) {
    const int gl = cell / p, pl = cell - gl * p;
    const double pm = gas[gl * HO_N + pl];
    gas[gl * HO_N + pl] = (s_gc[gl] > 0 && s_pc[pl] > 0) ? pm / ((double)s_gc[gl] + (double)s_pc[pl] - pm) : 0.0;
  }
  __syncthreads();

  // ---- 2: assignment, one wave per frame --------------------------------------------------------------------------------------------------
  {
    int* w_inter = reinterpret_cast<int*>(ho_lds + HO_LDS_WAVE + wave * HO_LDS_PER_WAVE);   // [row][column] of the frame's problem
    int* w_rid = w_inter + HO_N * HO_N;                            // class-local id of row r / column j, and their areas
    int* w_cid = w_rid + HO_N;
    int* w_ra = w_cid + HO_N;
    int* w_ca = w_ra + HO_N;
    for (int t = wave; t < T; t += HO_WAVES) {
      // the present ids of both sides, in ascending order (the lane's rank among the set bits below it)
      const int ag = lane < g ? gt_area[(long long)gid[lane] * T + t] : 0;
      const int ap = lane < p ? tr_area[(long long)pid[lane] * T + t] : 0;
      const unsigned long long mg = __ballot(ag > 0), mp = __ballot(ap > 0);
      const int ng = __popcll(mg), np = __popcll(mp);
      const unsigned long long below = (1ull << lane) - 1ull;
      const bool gt_rows = ng <= np;                               // the smaller side on the rows
      const int nr = gt_rows ? ng : np, nc = gt_rows ? np : ng;
      if (nr > 0) {
        if (ag > 0) {
          const int k = __popcll(mg & below);
          (gt_rows ? w_rid : w_cid)[k] = lane;
          (gt_rows ? w_ra : w_ca)[k] = ag;
        }
        if (ap > 0) {
          const int k = __popcll(mp & below);
          (gt_rows ? w_cid : w_rid)[k] = lane;
          (gt_rows ? w_ca : w_ra)[k] = ap;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane < nc) {
          const int cj = w_cid[lane];
          for (int r = 0; r < nr; ++r) {
            const int gl = gt_rows ? w_rid[r] : cj, pl = gt_rows ? cj : w_rid[r];
            w_inter[r * HO_N + lane] = inter[((long long)pid[pl] * G + gid[gl]) * T + t];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int cj = lane < nc ? w_cid[lane] : 0, ca = lane < nc ? w_ca[lane] : 1;
        auto sim_of = [&](int r) { return ho_sim(w_inter[r * HO_N + lane], w_ra[r], ca); };
        auto cost = [&](int r, int) {
          const int ri = w_rid[r];
          const double a = gt_rows ? gas[ri * HO_N + cj] : gas[cj * HO_N + ri];
          return -(a * sim_of(r));
        };
        int row4col;
        const int col4row = lsa_wave(nr, nc, lane, cost, row4col);
        // lane as row r / as column j -> the ground truth's lane
        if (gt_rows) {
          if (lane < nr && col4row >= 0 && col4row < nc) {
            const int gl = w_rid[lane], inter_rc = w_inter[lane * HO_N + col4row];
            my_match_col[(long long)t * g + gl] = inter_rc > 0 ? w_cid[col4row] : -1;
          }
        } else {
          if (lane < nc && row4col >= 0 && row4col < nr) {
            const int inter_rc = w_inter[row4col * HO_N + lane];
            my_match_col[(long long)t * g + cj] = inter_rc > 0 ? w_rid[row4col] : -1;
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                            // (the lists are rewritten for the wave's next frame)
      }
    }
  }
  __threadfence_block();
  __syncthreads();

  // ---- 3: tally, one lane per threshold -------------------------------------------------------------------------------------------------
  if (tid < A) {
    const double th = thr[tid];
    int tp = 0, fn = 0, fp = 0;
    double loca = 0.0;
    int* m = my_matches + (long long)tid * g * p;
    for (int t = 0; t < T; ++t) {
      int ng = 0, np = 0, num = 0;
      for (int pl = 0; pl < p; ++pl) np += tr_area[(long long)pid[pl] * T + t] > 0;
      double part = 0.0;
      for (int gl = 0; gl < g; ++gl) {
        const int ag = gt_area[(long long)gid[gl] * T + t];
        if (ag <= 0) continue;
        ++ng;
        const int pl = np > 0 ? my_match_col[(long long)t * g + gl] : -1;
        if (pl < 0 || pl >= p) continue;
        const double sim = ho_sim(inter[((long long)pid[pl] * G + gid[gl]) * T + t], ag, tr_area[(long long)pid[pl] * T + t]);
        if (sim >= th) {
          ++num;
          part += sim;
          m[gl * p + pl] += 1;
        }
      }
      tp += num;
      fn += ng - num;
      fp += np - num;
      if (num > 0) loca += part;
    }
    int* o = tp_fn_fp + ((long long)c * A + tid) * 3;
    o[0] = tp;
    o[1] = fn;
    o[2] = fp;
    loca_sum[(long long)c * A + tid] = loca;
  }
}

int hota_counts(const int* inter, const int* gt_area, const int* tr_area, int D, int G, int T, const int* gt_ids, const int* gt_starts,
                const int* tr_ids, const int* tr_starts, int C, int max_g, int max_p, const double* thr, int A, int* tp_fn_fp, int* matches,
                double* loca_sum, int* gt_id_count, int* tracker_id_count, int* match_col, hipStream_t st) {
  if (max_g > HO_N || max_p > HO_N || A > HO_A_MAX || T > 65535 || (long long)D * G * T >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  launch_lds(&hota_count_kernel, dim3((unsigned)C), (size_t)HO_LDS_TOTAL, st, inter, gt_area, tr_area, D, G, T, gt_ids, gt_starts, tr_ids,
             tr_starts, thr, A, tp_fn_fp, matches, loca_sum, gt_id_count, tracker_id_count, match_col);
  return check_launch("hota_counts");
}

// The solver alone: B problems, one wave each.  score: float64 [B, 64, 64] (row pitch 64); problem b is its top-left rows[b] x cols[b]
// corner and is MAXIMISED.  col_of_row: int32 [B, 64], the column of every row below rows[b] (-1 for the rows left over when
// rows[b] > cols[b]); the rest is not written.
__global__ __launch_bounds__(256) void lsa_max_kernel(const double* __restrict__ score, const int* __restrict__ rows,
                                                      const int* __restrict__ cols, int B, int* __restrict__ col_of_row) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * HO_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;                                              // (the whole wave; no workgroup barrier below)
  const int R = rows[b], Cn = cols[b];
  if (R < 1 || Cn < 1 || R > HO_N || Cn > HO_N) return;
  const double* s = score + (long long)b * HO_N * HO_N;
  const bool plain = R <= Cn;                                      // the smaller side on the solver's rows
  const int nr = plain ? R : Cn, nc = plain ? Cn : R;
  auto cost = [&](int i, int j) { return plain ? -s[i * HO_N + j] : -s[j * HO_N + i]; };
  int row4col;
  const int col4row = lsa_wave(nr, nc, lane, cost, row4col);
  int* o = col_of_row + (long long)b * HO_N;
  if (plain) {
    if (lane < R) o[lane] = col4row;
  } else {
    if (lane < R) o[lane] = row4col;                               // (lane = the problem's row = the solver's column)
  }
}

int lsa_max_f64(const double* score, const int* rows, const int* cols, int B, int* col_of_row, hipStream_t st) {
  hipLaunchKernelGGL(lsa_max_kernel, dim3((unsigned)((B + HO_WAVES - 1) / HO_WAVES)), dim3(256), 0, st, score, rows, cols, B, col_of_row);
  return check_launch("lsa_max_f64");
}

}  // namespace univs
