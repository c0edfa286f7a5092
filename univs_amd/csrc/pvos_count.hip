// Everything the VIPOSeg panoptic-VOS scores (mask IoU and boundary IoU per tracked object and frame, univs_amd/evaluation/pvos.py)
// need from one video, for every id at once.  The reference builds, per object and frame, two binary planes and erodes each d times
// with a 3 x 3 kernel after a one-pixel zero border (univs/evaluation/eval_utils_viposeg.py:27-80, called from the object loop of
// univs/evaluation/pvos_evaluation.py:185-201), d = round(0.02 diagonal): thousands of full-plane passes per frame for six integers
// per object.
//
// gt / pred: uint8 [T, H, W] id maps.  counts: int32 [T, K, 6], zeroed by the caller; cell [t, k - 1] = (I, A_g, A_p, BI, B_g, B_p) of id
// k in frame t: pixels with gt == pred == k, gt == k, pred == k, and the same three restricted to boundary pixels (BI: boundary on both
// sides).  Ids 0 and above K are not counted, but they are labels like any other where uniformity is decided.
//
// d erosions by 3 x 3 are one erosion by (2 d + 1) x (2 d + 1), and the zero border makes everything beyond the image background.  A
// label map gives each pixel to exactly one id, so the pixel survives the erosion of ITS id exactly when the (2 d + 1)^2 window around
// it lies inside the image and holds one label: the boundary maps of all ids of a side are one bit per pixel, "the window is not
// uniform or leaves the image".  Whether it leaves the image is a comparison of coordinates, so cells outside the image need no
// sentinel.  Uniformity is separable: a row window is uniform where the run of equal labels that ends at its right end is at least 2 d
// long; a square window is uniform where 2 d + 1 consecutive row windows are, with equal centre labels.  Neither a per-object plane nor
// an eroded plane exists in memory.
//
// A workgroup of 256 threads owns a tile of 64 x 64 pixels of one frame.  It reads the two maps of the tile with a halo of d once, into
// LDS bytes (zero outside the image); a tile without an id of 1..K on either side returns there.  Pass 1: a lane takes a row of tile +
// halo and walks it once for both maps, a dword of four labels at a time, keeping the run lengths; for the 64 tile columns it writes
// the two "row window uniform" bits into one byte.  Pass 2: a wave takes 16 tile rows, a lane one column of them; it walks down 16 +
// 2 d rows keeping, per side, the number of consecutive rows with the bit set and the same centre label.  A lane adds its pixels to the
// LDS histogram [K][6] once per run of equal (gt, pred) labels down its column; the histogram is flushed once per workgroup with one
// global atomic per non-zero cell.  Integers only: the result does not depend on the order.
//
// LDS, with B = 64 + 2 d and the row pitch P = B rounded up to a multiple of 4 whose quarter is odd (pass 1 has a lane per ROW: an odd
// dword pitch spreads the lanes' reads over the banks; the bit bytes have a pitch of 68 for the same reason): labels 2 B P bytes, bits
// 68 B, histogram 24 K + 8.  d = 29 (720p): 30.3 + 8.3 KB + histogram, three or four workgroups per CU by K; d = 44 (1080p): 47.4 +
// 10.3 KB, two; d = 88 (4K) with K = 255: 117.1 + 16.3 + 6.1 KB = 139.5 KB of the 160 KB, one (arithmetic, not measured occupancies).
// PV_D_MAX = 88 is the d of a 4K frame.  The halo is read (B / 64)^2 times per pixel from L2; whether that or pass 1's half-empty
// waves bound the kernel is not measured.
#include "count_core.h"
#include "launchers.h"

namespace univs {

constexpr int PV_TILE = 64;
constexpr int PV_D_MAX = 88;
constexpr int PV_K_MAX = 255;
constexpr int PV_SEG = PV_TILE / 4;                               // tile rows per wave in pass 2
constexpr int PV_BIT_PITCH = PV_TILE + 4;                         // bytes; 17 dwords

// the carve-up of the dynamic LDS, in 4-byte words (host and device)
struct PvosLds {
  int B, P;                                                        // rows (= used columns) of tile + halo, row pitch in bytes
  int hist, flag, bits, eg, ep, total;
};
__host__ __device__ inline PvosLds pvos_lds(int d, int K) {
  PvosLds L;
  L.B = PV_TILE + 2 * d;
  L.P = (L.B + 3) & ~3;
  if (((L.P >> 2) & 1) == 0) L.P += 4;
  int o = 0;
  L.hist = o; o += 6 * K;
  L.flag = o; o += 2;
  L.bits = o; o += L.B * PV_BIT_PITCH / 4;
  L.eg = o; o += L.B * L.P / 4;
  L.ep = o; o += L.B * L.P / 4;
  L.total = o;
  return L;
}

// a lane's pixels of one (gt, pred) pair of labels down its column: n pixels, of which bg / bp / bb are boundary on the gt side, the
// result side, both
__device__ __forceinline__ void pv_flush(int* hist, int K, int g, int p, int n, int bg, int bp, int bb) {
  if (n == 0) return;
  if (g >= 1 && g <= K) {
    atomicAdd(&hist[(g - 1) * 6 + 1], n);
    if (bg) atomicAdd(&hist[(g - 1) * 6 + 4], bg);
    if (g == p) {
      atomicAdd(&hist[(g - 1) * 6 + 0], n);
      if (bb) atomicAdd(&hist[(g - 1) * 6 + 3], bb);
    }
  }
  if (p >= 1 && p <= K) {
    atomicAdd(&hist[(p - 1) * 6 + 2], n);
    if (bp) atomicAdd(&hist[(p - 1) * 6 + 5], bp);
  }
}

__global__ __launch_bounds__(256) void pvos_count_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                         int T, int H, int W, int d, int K, int tiles_x, int tiles_y,
                                                         int* __restrict__ counts) {
  extern __shared__ int pv_lds[];
  const PvosLds L = pvos_lds(d, K);
  const int B = L.B, P = L.P;
  int* hist = pv_lds + L.hist;
  int* flag = pv_lds + L.flag;
  unsigned char* bits = reinterpret_cast<unsigned char*>(pv_lds + L.bits);
  unsigned char* eg = reinterpret_cast<unsigned char*>(pv_lds + L.eg);
  unsigned char* ep = reinterpret_cast<unsigned char*>(pv_lds + L.ep);
  const int tid = threadIdx.x;

  int blk = blockIdx.x;
  const int tx = blk % tiles_x;
  blk /= tiles_x;
  const int ty = blk % tiles_y, t = blk / tiles_y;
  const int y0 = ty * PV_TILE, x0 = tx * PV_TILE;

  if (tid < 2) flag[tid] = 0;
  hist_zero_n(hist, 6 * K);                                        // (with the barrier)

  // ---- the labels of tile + halo, each byte of the two maps read once; zero outside the image and in the pitch's tail --------------
  const int frame = t * H * W;                                     // (T H W < 2^31)
  unsigned any = 0;
  for (int i = tid; i < B * P; i += 256) {
    const int ey = i / P, ex = i - ey * P;
    const int gy = y0 - d + ey, gx = x0 - d + ex;
    unsigned g = 0, p = 0;
    if (ex < B && gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int o = frame + gy * W + gx;
      g = gt[o];
      p = pred[o];
      any |= (unsigned)(g >= 1u && g <= (unsigned)K) | (unsigned)(p >= 1u && p <= (unsigned)K);
    }
    eg[i] = (unsigned char)g;
    ep[i] = (unsigned char)p;
  }
  any = wave_or(any);
  if ((tid & 63) == 0 && any) atomicOr(&flag[0], 1);
  __syncthreads();
  if (flag[0] == 0) return;                                        // (the whole workgroup) no id of 1..K in reach of the tile

  // ---- pass 1: per row of tile + halo, the bits "the labels of columns [c, c + 2 d] are equal" for the tile columns c ---------------
  const int d2 = 2 * d;
  for (int ey = tid; ey < B; ey += 256) {
    const unsigned* rg = reinterpret_cast<const unsigned*>(eg + ey * P);
    const unsigned* rp = reinterpret_cast<const unsigned*>(ep + ey * P);
    unsigned char* rb = bits + ey * PV_BIT_PITCH;
    unsigned pg = 256u, pp = 256u;                                 // the labels to the left: none yet
    int rung = 0, runp = 0;                                        // equal labels immediately to the left
    for (int j = 0; j < P / 4; ++j) {
      unsigned wg = rg[j], wp = rp[j];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const unsigned vg = wg & 255u, vp = wp & 255u;
        wg >>= 8;
        wp >>= 8;
        rung = vg == pg ? rung + 1 : 0;
        runp = vp == pp ? runp + 1 : 0;
        pg = vg;
        pp = vp;
        const int c = 4 * j + b - d2;                              // the window that ends here starts at tile column c
        if (c >= 0 && c < PV_TILE) rb[c] = (unsigned char)((rung >= d2 ? 1 : 0) | (runp >= d2 ? 2 : 0));
      }
    }
  }
  __syncthreads();

  // ---- pass 2: down the columns; the pixel of tile row r is decided at row r + 2 d of tile + halo ---------------------------------
  {
    const int cx = tid & 63, r0 = (tid >> 6) * PV_SEG;             // (r0 is uniform over the wave)
    const int gx = x0 + cx;
    const bool x_in = gx < W, x_inner = gx - d >= 0 && gx + d < W;
    const unsigned char* cg = eg + cx + d;
    const unsigned char* cp = ep + cx + d;
    unsigned pg = 256u, pp = 256u;
    int cntg = 0, cntp = 0;                                        // consecutive rows, this one included, with the bit and one centre label
    int kg = -1, kp = -1, n = 0, nbg = 0, nbp = 0, nbb = 0;        // the lane's current run of (gt, pred) labels
    for (int ey = r0; ey < r0 + PV_SEG + d2; ++ey) {
      const unsigned f = bits[ey * PV_BIT_PITCH + cx];
      const unsigned vg = cg[ey * P], vp = cp[ey * P];
      cntg = (f & 1u) ? (cntg > 0 && vg == pg ? cntg + 1 : 1) : 0;
      cntp = (f & 2u) ? (cntp > 0 && vp == pp ? cntp + 1 : 1) : 0;
      pg = vg;
      pp = vp;
      const int r = ey - d2;
      const int gy = y0 + r;
      if (r < r0 || gy >= H || !x_in) continue;
      const bool inner = x_inner && gy - d >= 0 && gy + d < H;
      const int bg = !(inner && cntg > d2), bp = !(inner && cntp > d2);
      const int g = cg[(ey - d) * P], p = cp[(ey - d) * P];        // the pixel's own labels
      if (g != kg || p != kp) {
        pv_flush(hist, K, kg, kp, n, nbg, nbp, nbb);
        kg = g;
        kp = p;
        n = nbg = nbp = nbb = 0;
      }
      ++n;
      nbg += bg;
      nbp += bp;
      nbb += bg & bp;
    }
    pv_flush(hist, K, kg, kp, n, nbg, nbp, nbb);
  }

  hist_flush_n(hist, 6 * K, counts + (size_t)t * K * 6);          // (with the barrier)
}

int pvos_counts(const unsigned char* gt, const unsigned char* pred, int T, int H, int W, int d, int K, int* counts, hipStream_t st) {
  const long long hw = (long long)H * W;                          // (< 2^62)
  if (d > PV_D_MAX || K > PV_K_MAX || hw >= (1LL << 31) || hw * T >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  const int tiles_x = (W + PV_TILE - 1) / PV_TILE, tiles_y = (H + PV_TILE - 1) / PV_TILE;
  const size_t lds = (size_t)pvos_lds(d, K).total * sizeof(int);
  launch_lds(&pvos_count_kernel, dim3((unsigned)(tiles_x * tiles_y * T)), lds, st, gt, pred, T, H, W, d, K, tiles_x, tiles_y, counts);
  return check_launch("pvos_counts");
}

}  // namespace univs
