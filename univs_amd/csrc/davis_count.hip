// Everything the DAVIS scores J (region similarity) and F (boundary measure) need from one video, for every pair of a ground-truth
// object and a result object at once (univs_amd/evaluation/davis.py).  The reference calls `db_eval_iou` and `f_measure` per pair and
// frame; each `f_measure` builds two boundary maps and dilates both full planes with a disk of radius r through OpenCV
// (univs/evaluation/davis2017_evaluation/davis2017/metrics.py:6-37, :57-119, :122-178; the pair loops are
// univs/evaluation/vos_davis_evaluation.py:198-239): 2 G P dilations per frame, of which only the boundary pixels of the other side
// are ever looked up.
//
// gt / pred: uint8 [T, H, W] id maps.  gt 255 is void; gt ids 1..G and pred ids 1..P are objects, everything else is background.  With
// use_void a void pixel is taken out of both sides (`mask & ~void`); without it the void pixels are plain gt background and the result
// is untouched there (the semi-supervised task passes no void mask).  All outputs are int32, zeroed by the caller:
//
//   region [G, P, T, 2]  (intersection, union) of gt object i and result object j in frame t
//   n_gt [G, T]          boundary pixels of gt object i (`_seg2bmap`);  n_fg [P, T] the same for result object j
//   match [G, P, T, 2]   (gt boundary pixels of i inside the dilated boundary of j, result boundary pixels of j inside the dilated
//                        boundary of i)
//
// The objects of one id map are disjoint, so a pixel and its east / south / south-east neighbours name at most four ids, and the
// boundary maps of ALL objects of a side are one bit set per pixel: bit k = "boundary pixel of object k + 1".  `_seg2bmap` marks a pixel
// of object k where seg_k differs from a neighbour, i.e. where the pixel's id differs from that neighbour's and k is one of the two.  The
// OR of the other side's bit sets over the disk around a pixel is that pixel's membership in every dilated boundary at once, so one pass
// serves all G P pairs and neither the boundary maps nor the dilated planes exist in memory.
//
// A workgroup of 256 threads owns a tile of 64 x 64 pixels of one frame.  It reads the two id maps of the tile with a halo of r (+ 1 to
// the east and south, for the neighbours) once, as masked ids, into LDS bytes; everything else works on that copy.  The region counts
// come from those bytes (one LDS atomic per run of equal (gt, result) cells among a lane's 16 consecutive pixels).  Then, per side: the
// tile's own boundary pixels go to a work list; if there is one, the OTHER side's bit sets over tile + halo are written to LDS words and
// the lanes take list entries in turn, OR-ing row spans of half-width floor(sqrt(r^2 - d^2)) from the centre row outwards, and stop
// once every id present in the tile has been met.  A tile without any object id returns after the load.  Counts are integers, added in
// LDS and flushed with one global atomic per non-zero counter, so the result does not depend on the order.
//
// LDS, with B = 64 + 2 r: ids 2 (B + 1) roundup4(B + 1) bytes, bit sets 4 B^2, work list 8 KB, counters 4 ((G + 1)(P + 1) + 2 G P +
// 2 (G + P)) bytes, spans and flags 4 (r + 9).  r = 8 (480p), G = P = 5: 13.6 + 25.6 + 8 + 0.4 KB = 48 KB, three workgroups per CU;
// r = 18 (1080p): 20.8 + 40 + 8 KB = 69 KB, two; r = 36 (4K) with G = P = 32: 38.4 + 74 + 8 + 13 KB = 134 KB of the 160 KB, one
// (arithmetic, not measured occupancies).  DV_R_MAX = 36 is the radius of a 4K frame; 37 would still fit, nothing calls for it.
#include "count_core.h"
#include "launchers.h"

namespace univs {

constexpr int DV_TILE = 64;
constexpr int DV_R_MAX = 36;
constexpr int DV_MAX_OBJ = 32;
constexpr int DV_LIST_WORDS = DV_TILE * DV_TILE / 2;               // 4096 uint16 entries

// the carve-up of the dynamic LDS, in 4-byte words (host and device)
struct DavisLds {
  int BW, EW, EH;                                                  // bit-set tile width (= height), id tile row pitch (bytes) and rows
  int spans, flags, hist, m0, m1, ngt, nfg, ag, ap, zero_end, bits, list, eg, ep, total;
};
__host__ __device__ inline DavisLds davis_lds(int r, int G, int P) {
  DavisLds L;
  L.BW = DV_TILE + 2 * r;
  L.EH = L.BW + 1;
  L.EW = (L.BW + 1 + 3) & ~3;
  int o = 0;
  L.flags = o; o += 8;                                             // [0, 1] list lengths, [2, 3] ids present per side, [4] any id at all
  L.hist = o; o += (G + 1) * (P + 1);
  L.m0 = o; o += G * P;
  L.m1 = o; o += G * P;
  L.ngt = o; o += G;
  L.nfg = o; o += P;
  L.ag = o; o += G;
  L.ap = o; o += P;
  L.zero_end = o;
  L.spans = o; o += r + 1;
  L.bits = o; o += L.BW * L.BW;
  L.list = o; o += DV_LIST_WORDS;
  L.eg = o; o += L.EH * L.EW / 4;
  L.ep = o; o += L.EH * L.EW / 4;
  L.total = o;
  return L;
}

__device__ __forceinline__ unsigned dv_bit(unsigned v) { return v ? 1u << (v - 1) : 0u; }

// the boundary bit set of the image pixel (gy, gx), whose id lies at `q` in an id tile of row pitch EW (metrics.py:154-165: east, south
// and south-east; the last row compares east only, the last column south only, the bottom-right pixel nothing)
__device__ __forceinline__ unsigned dv_bits_at(const unsigned char* q, int EW, int gy, int gx, int H, int W) {
  const unsigned c = q[0];
  const bool east = gx + 1 < W, south = gy + 1 < H;
  unsigned b = 0;
  if (east) {
    const unsigned e = q[1];
    if (e != c) b |= dv_bit(c) | dv_bit(e);
  }
  if (south) {
    const unsigned s = q[EW];
    if (s != c) b |= dv_bit(c) | dv_bit(s);
  }
  if (east && south) {
    const unsigned se = q[EW + 1];
    if (se != c) b |= dv_bit(c) | dv_bit(se);
  }
  return b;
}

__global__ __launch_bounds__(256) void davis_count_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pred,
                                                          int T, int H, int W, int G, int P, int r, int use_void, int tiles_x,
                                                          int tiles_y, int* __restrict__ region, int* __restrict__ n_gt,
                                                          int* __restrict__ n_fg, int* __restrict__ match) {
  extern __shared__ int dv_lds[];
  const DavisLds L = davis_lds(r, G, P);
  const int BW = L.BW, EW = L.EW;
  int* flags = dv_lds + L.flags;
  int* hist = dv_lds + L.hist;
  int* spans = dv_lds + L.spans;
  unsigned* bits = reinterpret_cast<unsigned*>(dv_lds + L.bits);
  unsigned short* list = reinterpret_cast<unsigned short*>(dv_lds + L.list);
  unsigned char* eg = reinterpret_cast<unsigned char*>(dv_lds + L.eg);
  unsigned char* ep = reinterpret_cast<unsigned char*>(dv_lds + L.ep);
  const int tid = threadIdx.x;

  int blk = blockIdx.x;
  const int tx = blk % tiles_x;
  blk /= tiles_x;
  const int ty = blk % tiles_y, t = blk / tiles_y;
  const int y0 = ty * DV_TILE, x0 = tx * DV_TILE;

  for (int i = tid; i < L.zero_end; i += 256) dv_lds[i] = 0;
  if (tid <= r) {                                                  // floor(sqrt(r^2 - d^2)) in integers
    int w = r;
    while (w * w + tid * tid > r * r) --w;
    spans[tid] = w;
  }
  __syncthreads();

  // ---- the masked ids of tile + halo, each byte of the two maps read once ----------------------------------------------------------
  const int frame = t * H * W;                                     // (T H W < 2^31)
  unsigned any = 0;
  for (int i = tid; i < L.EH * EW; i += 256) {
    const int ey = i / EW, ex = i - ey * EW;
    const int gy = y0 - r + ey, gx = x0 - r + ex;
    unsigned g = 0, p = 0;
    if (ex <= BW && gy >= 0 && gy < H && gx >= 0 && gx < W) {
      const int o = frame + gy * W + gx;
      g = gt[o];
      p = pred[o];
      const bool v = g == 255u;
      if (g > (unsigned)G) g = 0;
      if (p > (unsigned)P || (v && use_void)) p = 0;
    }
    eg[i] = (unsigned char)g;
    ep[i] = (unsigned char)p;
    any |= g | p;
  }
  any = wave_or(any);
  if ((tid & 63) == 0 && any) atomicOr(&flags[4], 1);
  __syncthreads();
  if (flags[4] == 0) return;                                       // (the whole workgroup) nothing but background and void

  // ---- region counts: the lane's 16 consecutive pixels of one row, one LDS atomic per run of equal cells ---------------------------
  const int row = tid >> 2, seg = (tid & 3) * 16;
  const int cgy = y0 + row;
  const int nx = cgy < H ? min(16, W - (x0 + seg)) : 0;            // the lane's pixels inside the image (may be <= 0)
  const unsigned char* cg = eg + (row + r) * EW + seg + r;
  const unsigned char* cp = ep + (row + r) * EW + seg + r;
  {
    int prev = 0, run = 0;
    for (int k = 0; k < nx; ++k) {
      const int cell = (int)cg[k] * (P + 1) + (int)cp[k];
      if (cell != prev) {
        if (prev && run) atomicAdd(&hist[prev], run);
        prev = cell;
        run = 0;
      }
      ++run;
    }
    if (prev && run) atomicAdd(&hist[prev], run);
  }

  // ---- side 0: the gt boundary pixels against the dilated result boundaries; side 1: the mirror image ------------------------------
  for (int side = 0; side < 2; ++side) {
    const unsigned char* own = side == 0 ? eg : ep;
    const unsigned char* oth = side == 0 ? ep : eg;
    const unsigned char* co = side == 0 ? cg : cp;
    int* n_own = dv_lds + (side == 0 ? L.ngt : L.nfg);
    int* mm = dv_lds + (side == 0 ? L.m0 : L.m1);
    for (int k = 0; k < nx; ++k)
      if (dv_bits_at(co + k, EW, cgy, x0 + seg + k, H, W)) list[atomicAdd(&flags[side], 1)] = (unsigned short)(row * DV_TILE + seg + k);
    __syncthreads();
    const int n = flags[side];
    if (n == 0) continue;                                          // (the whole workgroup)
    unsigned seen = 0;
    for (int i = tid; i < BW * BW; i += 256) {
      const int by = i / BW, bx = i - by * BW;
      const int gy = y0 - r + by, gx = x0 - r + bx;
      unsigned b = 0;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) b = dv_bits_at(oth + by * EW + bx, EW, gy, gx, H, W);
      bits[i] = b;
      seen |= b;
    }
    seen = wave_or(seen);
    if ((tid & 63) == 0 && seen) atomicOr(&flags[2 + side], (int)seen);
    __syncthreads();
    const unsigned present = (unsigned)flags[2 + side];
    for (int item = tid; item < n; item += 256) {
      const int pix = list[item], cy = pix >> 6, cx = pix & 63;
      unsigned ownb = dv_bits_at(own + (cy + r) * EW + cx + r, EW, y0 + cy, x0 + cx, H, W);
      const unsigned* c = bits + (cy + r) * BW + cx + r;
      unsigned acc = 0;
      for (int d = 0; d <= r && acc != present; ++d) {
        const int hw = spans[d];
        const unsigned* up = c - d * BW;
        const unsigned* dn = c + d * BW;
        for (int dx = -hw; dx <= hw; ++dx) acc |= up[dx] | dn[dx];
      }
      while (ownb) {
        const int a = __ffs((int)ownb) - 1;
        ownb &= ownb - 1;
        atomicAdd(&n_own[a], 1);
        unsigned m = acc;
        while (m) {
          const int b = __ffs((int)m) - 1;
          m &= m - 1;
          atomicAdd(&mm[side == 0 ? a * P + b : b * P + a], 1);
        }
      }
    }
    __syncthreads();                                               // the list and the bit sets are rewritten for the other side
  }

  // ---- flush --------------------------------------------------------------------------------------------------------------------------
  __syncthreads();
  int* ag = dv_lds + L.ag;
  int* ap = dv_lds + L.ap;
  if (tid < G) {
    int s = 0;
    for (int j = 0; j <= P; ++j) s += hist[(tid + 1) * (P + 1) + j];
    ag[tid] = s;
  } else if (tid >= 64 && tid < 64 + P) {
    int s = 0;
    for (int i = 0; i <= G; ++i) s += hist[i * (P + 1) + tid - 64 + 1];
    ap[tid - 64] = s;
  }
  __syncthreads();
  const int* m0 = dv_lds + L.m0;
  const int* m1 = dv_lds + L.m1;
  for (int idx = tid; idx < G * P; idx += 256) {
    const int i = idx / P, j = idx - i * P;
    const int inter = hist[(i + 1) * (P + 1) + j + 1], uni = ag[i] + ap[j] - inter;
    const size_t o = ((size_t)idx * T + t) * 2;
    if (inter) atomicAdd(region + o, inter);
    if (uni) atomicAdd(region + o + 1, uni);
    if (m0[idx]) atomicAdd(match + o, m0[idx]);
    if (m1[idx]) atomicAdd(match + o + 1, m1[idx]);
  }
  const int* ngt = dv_lds + L.ngt;
  const int* nfg = dv_lds + L.nfg;
  if (tid < G) {
    if (ngt[tid]) atomicAdd(n_gt + (size_t)tid * T + t, ngt[tid]);
  } else if (tid >= 64 && tid < 64 + P) {
    if (nfg[tid - 64]) atomicAdd(n_fg + (size_t)(tid - 64) * T + t, nfg[tid - 64]);
  }
}

int davis_counts(const unsigned char* gt, const unsigned char* pred, int T, int H, int W, int G, int P, int radius, int use_void,
                 int* region, int* n_gt, int* n_fg, int* match, hipStream_t st) {
  const long long hw = (long long)H * W;                          // (< 2^62)
  if (G > DV_MAX_OBJ || P > DV_MAX_OBJ || radius > DV_R_MAX || hw >= (1LL << 31) || hw * T >= (1LL << 31)) return UNIVS_ERR_NOT_IMPLEMENTED;
  const int tiles_x = (W + DV_TILE - 1) / DV_TILE, tiles_y = (H + DV_TILE - 1) / DV_TILE;
  const size_t lds = (size_t)davis_lds(radius, G, P).total * sizeof(int);
  launch_lds(&davis_count_kernel, dim3((unsigned)(tiles_x * tiles_y * T)), lds, st, gt, pred, T, H, W, G, P, radius, use_void, tiles_x, tiles_y,
             region, n_gt, n_fg, match);
  return check_launch("davis_counts");
}

}  // namespace univs
