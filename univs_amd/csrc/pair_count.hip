// The per-frame pair table of a video panoptic evaluation: counts[t][g][p] = the pixels of frame t whose ground-truth segment id is
// gt_ids[g] and whose predicted segment id is pred_ids[p].  VPQ (every window of every length) and STQ are sums over these tables
// (univs_amd/evaluation/vps.py); the reference re-reads and sorts the pixels of a frame once per window it is part of
// (univs/evaluation/eval_vpq_vps.py:83-165, eval_stq_vps.py:134-161, eval_stquality_vps.py:111-195).
//
// Either side is uint8 [T, H, W, 3] (the decoded PNG: id = R + 256 G + 65536 B) or int32 [T, H, W] (an id map).  Row / column G / P of
// a table is the bucket of the ids that are not listed; first_unknown[t][side] is the largest such id (-1: none that is >= 0).
//
// grid (row segments, T), 256 threads.  Both id tables and the (G + 1)(P + 1) histogram live in LDS.  A lane takes four consecutive
// pixels: whole dwords of the RGB rows (12 bytes = 3 dwords, shifted by the row segment's byte alignment), never byte loads.  It maps
// an id by binary search in LDS and keeps the last (id, index) of each side in registers: panoptic maps are long runs, so most pixels
// skip the search.  When the whole wave holds one pair, one lane adds 256; otherwise a lane adds each of its runs with one LDS atomic.
// (count_core.h: hist_add4).  The histogram reaches global memory once per workgroup (mask_post.h: hist_flush_n).
#include "count_core.h"
#include "launchers.h"

namespace univs {

constexpr int PAIR_MAX_IDS = 1024;      // G, P
constexpr int PAIR_MAX_CELLS = 16384;   // (G + 1)(P + 1): a 64 KB histogram + at most 8 KB of id tables, so two workgroups fit the 160 KB
                                        // of LDS of a gfx950 CU (arithmetic, not a measured occupancy)

struct __attribute__((packed, aligned(4))) Words4 {
  unsigned w[4];
};

// the ids of pixels [p, p + 4) of a segment that starts at byte address `seg`; n of them exist.  `end`: the end of the whole buffer
// rounded up to a dword (no load starts at or beyond it; the buffer's base is dword-aligned).
template <bool RGB>
__device__ __forceinline__ void load_ids4(const unsigned char* seg, const unsigned char* end, long long p, int n, int (&id)[4]) {
  const unsigned char* at = seg + p * (RGB ? 3 : 4);
  const unsigned a = RGB ? (unsigned)((uintptr_t)at & 3) : 0u;
  const unsigned char* w0 = at - a;
  unsigned w[4];
  if (w0 + 16 <= end) {
    const Words4 v = *reinterpret_cast<const Words4*>(w0);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = v.w[i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = w0 + 4 * i < end ? *reinterpret_cast<const unsigned*>(w0 + 4 * i) : 0u;
  }
  if constexpr (RGB) {
    const unsigned sh = 8 * a;
    unsigned d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = (unsigned)(((((unsigned long long)w[i + 1]) << 32) | w[i]) >> sh);
    id[0] = (int)(d[0] & 0xFFFFFFu);
    id[1] = (int)((d[0] >> 24) | ((d[1] & 0xFFFFu) << 8));
    id[2] = (int)((d[1] >> 16) | ((d[2] & 0xFFu) << 16));
    id[3] = (int)(d[2] >> 8);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) id[i] = (int)w[i];
  }
  (void)n;
}

// the position of `id` in the ascending table tab[n] (LDS), n where it is absent; `last_id` / `last_idx`: the lane's previous answer
// (last_idx < 0: none yet); `unknown`: the largest absent id seen
__device__ __forceinline__ int table_index(const int* tab, int n, int id, int& last_id, int& last_idx, int& unknown) {
  if (last_idx >= 0 && id == last_id) return last_idx;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  const int idx = (lo < n && tab[lo] == id) ? lo : n;
  if (idx == n) unknown = max(unknown, id);
  last_id = id;
  last_idx = idx;
  return idx;
}

template <bool GRGB, bool PRGB>
__global__ __launch_bounds__(256) void pair_count_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                         const unsigned char* gt_end, const unsigned char* pred_end, int H, int W,
                                                         int rows_per_seg, const int* __restrict__ gt_ids, int G,
                                                         const int* __restrict__ pred_ids, int P, int* __restrict__ counts,
                                                         int* __restrict__ first_unknown) {
  extern __shared__ int pair_lds[];                               // gt table [G], pred table [P], histogram [(G + 1)(P + 1)]
  int* gtab = pair_lds;
  int* ptab = pair_lds + G;
  int* hist = pair_lds + G + P;
  const int cells = (G + 1) * (P + 1);
  const int t = blockIdx.y;
  const int y0 = blockIdx.x * rows_per_seg, y1 = min(H, y0 + rows_per_seg);
  if (y0 >= y1) return;                                           // (the whole workgroup)
  for (int i = threadIdx.x; i < G; i += 256) gtab[i] = gt_ids[i];
  for (int i = threadIdx.x; i < P; i += 256) ptab[i] = pred_ids[i];
  hist_zero_n(hist, cells);                                       // (and the barrier behind the tables)

  const long long first = ((long long)t * H + y0) * W;            // the segment's first pixel in the whole buffer
  const unsigned char* gseg = gt + first * (GRGB ? 3 : 4);
  const unsigned char* pseg = pred + first * (PRGB ? 3 : 4);
  const int npix = (y1 - y0) * W;
  const int groups = (npix + 3) >> 2;
  int g_id = 0, g_idx = -1, p_id = 0, p_idx = -1, g_unknown = -1, p_unknown = -1;
  for (int base = 0; base < groups; base += 256) {                // (a uniform trip count: the ballot sees every lane)
    const int grp = base + threadIdx.x;
    const int n = grp < groups ? min(4, npix - 4 * grp) : 0;
    int a[4], b[4], cell[4];
    if (n > 0) {
      load_ids4<GRGB>(gseg, gt_end, 4LL * grp, n, a);
      load_ids4<PRGB>(pseg, pred_end, 4LL * grp, n, b);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cell[j] = -1;
      if (j < n) {
        const int gi = table_index(gtab, G, a[j], g_id, g_idx, g_unknown);
        const int pi = table_index(ptab, P, b[j], p_id, p_idx, p_unknown);
        cell[j] = gi * (P + 1) + pi;
      }
    }
    hist_add4(hist, cell);
  }
  hist_flush_n(hist, cells, counts + (long long)t * cells);
  g_unknown = wave_max(g_unknown);
  p_unknown = wave_max(p_unknown);
  if ((threadIdx.x & 63) == 0) {
    if (g_unknown >= 0) atomicMax(first_unknown + 2 * t, g_unknown);
    if (p_unknown >= 0) atomicMax(first_unknown + 2 * t + 1, p_unknown);
  }
}

template <bool GRGB, bool PRGB>
static void launch_pair_count(const void* gt, const void* pred, int T, int H, int W, const int* gt_ids, int G, const int* pred_ids, int P,
                              int* counts, int* first_unknown, hipStream_t st) {
  int rps = 0;
  const int segs = row_segments(H, T, &rps);
  const size_t lds = ((size_t)G + P + (size_t)(G + 1) * (P + 1)) * sizeof(int);
  const long long px = (long long)T * H * W;
  const unsigned char* g = static_cast<const unsigned char*>(gt);
  const unsigned char* p = static_cast<const unsigned char*>(pred);
  const unsigned char* g_end = g + ((px * (GRGB ? 3 : 4) + 3) & ~3LL);
  const unsigned char* p_end = p + ((px * (PRGB ? 3 : 4) + 3) & ~3LL);
  launch_lds(&pair_count_kernel<GRGB, PRGB>, dim3((unsigned)segs, (unsigned)T), lds, st, g, p, g_end, p_end, H, W, rps, gt_ids, G, pred_ids, P,
             counts, first_unknown);
}

int panoptic_pair_counts(const void* gt, int gt_rgb, const void* pred, int pred_rgb, int T, int H, int W, const int* gt_ids, int G,
                         const int* pred_ids, int P, int* counts, int* first_unknown, hipStream_t st) {
  if (G > PAIR_MAX_IDS || P > PAIR_MAX_IDS || (long long)(G + 1) * (P + 1) > PAIR_MAX_CELLS || T > 65535 ||
      (long long)H * W > INT32_MAX || ((uintptr_t)gt & 3) || ((uintptr_t)pred & 3))
    return UNIVS_ERR_NOT_IMPLEMENTED;
  if (gt_rgb && pred_rgb) launch_pair_count<true, true>(gt, pred, T, H, W, gt_ids, G, pred_ids, P, counts, first_unknown, st);
  else if (gt_rgb) launch_pair_count<true, false>(gt, pred, T, H, W, gt_ids, G, pred_ids, P, counts, first_unknown, st);
  else if (pred_rgb) launch_pair_count<false, true>(gt, pred, T, H, W, gt_ids, G, pred_ids, P, counts, first_unknown, st);
  else launch_pair_count<false, false>(gt, pred, T, H, W, gt_ids, G, pred_ids, P, counts, first_unknown, st);
  return check_launch("panoptic_pair_counts");
}

}  // namespace univs
