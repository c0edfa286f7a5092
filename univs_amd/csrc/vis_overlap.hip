// The per-frame overlaps |d_t AND g_t| of every detection d and every ground truth g of one video, read off the run-length codes
// (univs_amd/evaluation/ytvis.py).  The reference fills ious[d, g] in a Python double loop whose cells call maskUtils.merge twice and
// maskUtils.area twice per frame (univs/data/datasets/ytvis_api/ytvoseval.py:173-219, `iou_seq` :200-214); its IoU of two sequences is
// I / (A_d + A_g - I) with I the sum of these overlaps over the frames and A the summed areas, so this table is all of computeIoU that
// touches a mask.  No mask is decoded.  Integers only.
//
// The two sides come in one layout (vis_counts.runs_from_rles).  `bounds`: the cumulative column-major run boundaries of all masks back
// to back; mask m owns bounds[starts[m] : starts[m + 1]], its run k covers [b_{k-1}, b_k) with b_{-1} = 0, odd runs are foreground,
// the last boundary is H W.  `ones[k]`: the foreground pixels of the mask in [0, b_k).  starts[m + 1] == starts[m]: the mask is absent
// (`None`), which counts as an empty one.  Detection masks are d T + t, ground-truth masks g T + t.
//
// A workgroup of 256 threads takes one (g, t) and `chunk` detections.  It stages g's bounds and ones in LDS once; each of its four
// waves then takes one detection of the chunk at a time.  The lanes stride over that detection's foreground runs [s, e), read from
// global memory, and add C(e) - C(s), where C(x) = the foreground of g in [0, x): a binary search in the staged bounds for the last
// b_k <= x gives ones[k], plus x - b_k when run k + 1 is foreground (k even).  Zero-length runs repeat a boundary; "the last b_k <= x"
// steps over them.  A wave reduction, and lane 0 stores the cell: every cell of inter [D, G, T] is written exactly once, by one plain
// store, so the caller need not zero it.  An absent or empty mask on either side stores 0, and so does a detection whose first-to-last
// foreground span does not meet g's -- before any search.  A ground-truth mask with more than `cap` boundaries (the caller states the
// largest count; the device array cannot be asked without a synchronisation) stores -1 in its cells and nothing is staged.
//
// LDS: 8 bytes per boundary of the largest ground-truth mask.  VO_MAX_BOUNDS = 16384 boundaries are 128 KB of the 160 KB of a CU -- one
// workgroup per CU there; a 720 x 1280 mask of a convex object has at most 2 x 1280 boundaries (20 KB, 8 workgroups).  Sums: a lane's
// and a wave's are at most H W < 2^31.
#include "count_core.h"
#include "launchers.h"

namespace univs {

constexpr int VO_MAX_BOUNDS = 16384;

// the foreground of the staged mask in [0, x): n >= 1 boundaries gb, their prefix counts go
__device__ __forceinline__ int vo_prefix(const int* gb, const int* go, int n, int x) {
  int lo = 0, hi = n;                                              // the number of boundaries <= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (gb[mid] <= x) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return 0;                                           // inside run 0: background
  const int k = lo - 1;
  return go[k] + ((k & 1) == 0 ? x - gb[k] : 0);
}

__global__ __launch_bounds__(256) void vis_overlap_kernel(const int* __restrict__ dt_bounds, const int* __restrict__ dt_starts,
                                                          const int* __restrict__ gt_bounds, const int* __restrict__ gt_ones,
                                                          const int* __restrict__ gt_starts, int D, int G, int T, int cap, int chunk,
                                                          int* __restrict__ inter) {
  extern __shared__ int vo_lds[];
  int* gb = vo_lds;
  int* go = vo_lds + cap;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = (int)blockIdx.x, t = (int)blockIdx.y, gm = g * T + t;   // (no division: its expansion goes through f32)
  const int d0 = (int)blockIdx.z * chunk, d1 = min(d0 + chunk, D);
  const int gs = gt_starts[gm], gn = gt_starts[gm + 1] - gs;

  // ---- nothing to search: g absent, empty, or larger than the caller said -----------------------------------------------------------
  const bool over = gn > cap;
  if (gn < 2 || over || gt_ones[gs + gn - 1] == 0) {               // (the whole workgroup; one boundary is the empty mask)
    for (int d = d0 + tid; d < d1; d += 256) inter[((size_t)d * G + g) * T + t] = over ? -1 : 0;
    return;
  }
  for (int i = tid; i < gn; i += 256) {
    gb[i] = gt_bounds[gs + i];
    go[i] = gt_ones[gs + i];
  }
  __syncthreads();
  // g's foreground lies in [g_lo, g_hi)
  const int g_lo = gb[0], g_hi = (gn & 1) ? gb[gn - 2] : gb[gn - 1];

  for (int d = d0 + wave; d < d1; d += 4) {                        // (uniform over the wave)
    const int dm = d * T + t;
    const int ds = dt_starts[dm], dn = dt_starts[dm + 1] - ds;
    const int* db = dt_bounds + ds;
    int acc = 0;
    if (dn >= 2) {
      const int d_lo = db[0], d_hi = (dn & 1) ? db[dn - 2] : db[dn - 1];
      if (d_lo < g_hi && d_hi > g_lo) {
        for (int j = 2 * lane + 1; j < dn; j += 128) {             // the foreground runs [db[j - 1], db[j])
          const int s = db[j - 1], e = db[j];
          if (e > s && s < g_hi && e > g_lo) acc += vo_prefix(gb, go, gn, e) - vo_prefix(gb, go, gn, s);
        }
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) inter[((size_t)d * G + g) * T + t] = acc;
  }
}

int vis_overlap_counts(const int* dt_bounds, const int* dt_starts, const int* gt_bounds, const int* gt_ones, const int* gt_starts, int D,
                       int G, int T, int H, int W, int gt_max_bounds, int* inter, hipStream_t st) {
  if ((long long)H * W >= (1LL << 31) || gt_max_bounds > VO_MAX_BOUNDS || T > 65535) return UNIVS_ERR_NOT_IMPLEMENTED;   // (T: grid.y)
  // about four workgroups per CU; a chunk is a multiple of the four waves
  const long long gt = (long long)G * T;                           // (D G T < 2^31: the entry's check)
  const long long across = std::max<long long>(1, 4LL * cu_count() / gt);
  int chunk = (int)((D + across - 1) / across);
  chunk = (chunk + 3) & ~3;
  const int chunks = (D + chunk - 1) / chunk;                      // (<= `across` <= 4 CUs < 65536: grid.z)
  launch_lds(&vis_overlap_kernel, dim3((unsigned)G, (unsigned)T, (unsigned)chunks), (size_t)gt_max_bounds * 2 * sizeof(int), st, dt_bounds, dt_starts,
             gt_bounds, gt_ones, gt_starts, D, G, T, gt_max_bounds, chunk, inter);
  return check_launch("vis_overlap_counts");
}

}  // namespace univs
