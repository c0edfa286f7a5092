// What the LDS-windowed MSDA kernels with per-tile piece lists share (msda_strips.hip: generation 5, msda_heads.hip:
// generation 6): the sample-record helpers, the tile header, the host container and ONE table builder, parametrised by a
// small per-generation traits struct (msda_strips_geom.h: S5Geom, msda_heads_geom.h: S6Geom).  Pure C++ plus
// __host__ __device__ inlines, no HIP calls: the host emulators (tools/strips_emulate.cpp, tools/heads_emulate.cpp) build
// the very tables and records the kernels read.
//
// Geometry.  Tiles of TW x TH queries of the finest level (plus the queries of the coarser levels whose reference points
// fall into the tile), numbered column-major: tile = tx * tiles_y + ty, so consecutive tiles are vertical neighbours and a
// workgroup walks down a tile column.  Every level's window of a tile (bilinear footprints of samples within R pixels of
// the tile's box, plus the one-pixel zero ring around the level) is resident in LDS, one region per level, its rows
// circular: moving one tile down replaces only the rows that left the window.  A generation chooses how level rows map to
// LDS rows (G::ROW_SHIFT) and how wide a row piece is (G::BLOCK); its header describes the resulting address.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>

#include "msda_geometry.h"

namespace univs {

constexpr int WIN_LMAX = 4;

// Slot order of the levels (the order the kernels visit them in, and the order of the levels in the head-major projection
// layout: ops.msda_level_order builds it with the same rule): by size, largest first, ties by index.
static inline void win_slot_order(const LevelTable& lv, int L, int* ord) {
  for (int l = 0; l < L; ++l) ord[l] = l;
  std::sort(ord, ord + L, [&](int a, int b) {
    const long long sa = (long long)lv.H[a] * lv.W[a], sb = (long long)lv.H[b] * lv.W[b];
    return sa != sb ? sa > sb : a < b;
  });
}

// Per tile, workgroup-uniform; 16 dwords, fetched with one vector load (lane k = dword k & 15).
struct WinTile {
  // p0: (wx0 + 1) | (wy0 + 1) << 12 | rot << 24 | par << 30 -- first column / row of the tile's window (zero ring included:
  // >= -1), rot = LDS row of the window's first row, par = which of the level rows sharing that LDS row it is (always 0
  // when G::ROW_SHIFT == 0);  p1: (ww - 2) | (wh - 2) << 8 -- the upper-left corner of a footprint may sit in window
  // columns [0, ww - 2], rows [0, wh - 2]
  unsigned p0[WIN_LMAX], p1[WIN_LMAX];
  int total;     // queries of the tile
  int n_cold;    // pieces per wave of this tile's "whole windows" list
  int n_enter;   // pieces per wave of an "entering rows" list (rows a tile's windows have and the windows of the tile above
                 // it -- ty - 1 of the same column -- have not; the whole windows at the top of a column): this tile's own,
                 // or with G::ENTER_OF_NEXT that of the NEXT tile in the sequence (wrapping)
  int pad[5];
};
static_assert(sizeof(WinTile) == 64, "16 dwords");
__host__ __device__ __forceinline__ int win_wx0(unsigned p0) { return (int)(p0 & 0xfffu) - 1; }
__host__ __device__ __forceinline__ int win_wy0(unsigned p0) { return (int)((p0 >> 12) & 0xfffu) - 1; }
__host__ __device__ __forceinline__ int win_rot(unsigned p0) { return (int)((p0 >> 24) & 0x3fu); }

// ---- a lane's sample record at one level (s5_record / s6_record fill it: the addresses are the generation's own).
// The LDS byte addresses of the four corners in the lane's visiting order (chunk rotation already in the address bits: read
// chunk slot j at a[k] ^ (j << 4)) with their weights, and `inwin`: the footprint lies inside the window (otherwise all
// weights are 0, the addresses point at the window's first pixel, and the caller checks whether the sample is inside the
// band and adds it from global memory).
struct WinRec {
  unsigned a[4];
  float w[4];
  bool inwin;
};
__host__ __device__ __forceinline__ int win_floor_to_int(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(v));   // floor and convert in one (saturating)
  return r;
#else
  return (int)floorf(fminf(fmaxf(v, -1e6f), 1e6f));
#endif
}
__host__ __device__ __forceinline__ unsigned win_mul24(unsigned a, unsigned b) {   // both < 2^24
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(a, b);
#else
  return a * b;
#endif
}
__host__ __device__ __forceinline__ float win_fract(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_fractf(v);                      // v - floor(v), kept below 1
#else
  return v - floorf(v);
#endif
}
// inside the reference's band (-1, H) x (-1, W)?  (only evaluated for samples outside the window: the rare path)
__host__ __device__ __forceinline__ bool win_inband(float x, float y, float Hf, float Wf) {
  const float him = fmaf(y, Hf, -0.5f), wim = fmaf(x, Wf, -0.5f);
  return him > -1.f && wim > -1.f && him < Hf && wim < Wf;
}

template <class G>
struct WinHost {
  typename G::Levels lv;
  std::vector<WinTile> tiles;               // [ntiles]
  std::vector<typename G::Piece> pieces;    // [ntiles][2][G::NW][G::PCAP]: list 0 = entering rows, list 1 = whole windows
  std::vector<int> qtab;                    // [ntiles][G::QCAP]: global query index of the tile's i-th query (padded with the last)
  int ntiles = 0, tiles_x = 0, tiles_y = 0;
  long long qmax = 0;                       // max queries of a tile
  size_t lds = 0;                           // bytes of all the levels' circular windows
  bool ok = false;                          // the tables fit their caps
};

static inline int win_pos_mod(int a, int b) { return ((a % b) + b) % b; }

// The tables of one (level shapes, tile, halo).  fine = index of the largest level.  Returns g.ok.  G supplies
//   Levels, Piece             the kernel-facing structs; ROWS = the member of Levels that holds the LDS rows of a region
//   NW, QCAP, PCAP            waves per workgroup, queries per tile, pieces per wave and list
//   ROWS_MAX, PITCH_MAX       window caps (rows, pixels)
//   BLOCK, PX_BIAS, pack()   pixels of a row piece, the bias of its pixel index, its packing
//   ROW_SHIFT                 1 << ROW_SHIFT consecutive level rows (by Y = y + 1 >= 0) share one LDS row of pitch * 128 bytes,
//                             each with 128 >> ROW_SHIFT bytes per pixel
//   ENTER_OF_NEXT             WinTile::n_enter is the next tile's count (the kernel stages a tile ahead) or the tile's own
//   MONOTONIC                 refuse tables whose windows do not move down monotonically within a column
template <class G>
static bool win_build_host(const LevelTable& lv, int L, int fine, int TH, int TW, int R, WinHost<G>& g) {
  g = WinHost<G>();
  if (L < 1 || L > WIN_LMAX || TH < 1 || TW < 1) return false;
  constexpr int SUB = (1 << G::ROW_SHIFT) - 1, SUB_BYTES = 128 >> G::ROW_SHIFT;
  const int tiles_y = (lv.H[fine] + TH - 1) / TH, tiles_x = (lv.W[fine] + TW - 1) / TW;
  g.tiles_x = tiles_x; g.tiles_y = tiles_y;
  std::vector<int4> ax((size_t)L * tiles_x), ay((size_t)L * tiles_y);
  int pitch[UNIVS_MAX_LEVELS] = {0, 0, 0, 0}, nrow[UNIVS_MAX_LEVELS] = {0, 0, 0, 0};
  for (int l = 0; l < L; ++l) {
    int mw = 2, mr = 1;
    for (int tx = 0; tx < tiles_x; ++tx) {
      int4& e = ax[(size_t)l * tiles_x + tx];
      axis_entry(tx, tiles_x, TW, lv.W[l], lv.W[fine], R, G::PITCH_MAX, /*ring=*/1, e);
      mw = std::max(mw, e.w);
    }
    for (int ty = 0; ty < tiles_y; ++ty) {
      int4& e = ay[(size_t)l * tiles_y + ty];
      axis_entry(ty, tiles_y, TH, lv.H[l], lv.H[fine], R, G::ROWS_MAX, /*ring=*/1, e);
      const int Yf = e.z + 1, Yl = e.z + e.w;          // first / last window row, shifted by the ring
      mr = std::max(mr, (Yl >> G::ROW_SHIFT) - (Yf >> G::ROW_SHIFT) + 1);
    }
    pitch[l] = (mw + 1) & ~1;                          // even
    nrow[l] = mr;
  }
  int ord[UNIVS_MAX_LEVELS];
  win_slot_order(lv, L, ord);
  g.ntiles = tiles_y * tiles_x;
  g.ok = true;
  std::memset(&g.lv, 0, sizeof(g.lv));
  size_t lds = 0;
  for (int kk = 0; kk < L; ++kk) {
    const int l = ord[kk];
    g.lv.H[kk] = lv.H[l]; g.lv.W[kk] = lv.W[l]; g.lv.start[kk] = lv.start[l]; g.lv.l[kk] = l;
    g.lv.pitch[kk] = pitch[l]; (g.lv.*G::ROWS)[kk] = nrow[l]; g.lv.reg[kk] = (int)lds;
    g.lv.rW[kk] = 1.0f / (float)lv.W[l]; g.lv.rH[kk] = 1.0f / (float)lv.H[l];
    // byte distance from a level row that is the LAST of its LDS row (at + SUB * SUB_BYTES) to the one below it, in the next
    // LDS row or wrapping to LDS row 0 -- less the SUB * SUB_BYTES between two rows of one LDS row, which the record always adds
    g.lv.next_d[kk] = pitch[l] * 128 - 2 * SUB * SUB_BYTES;
    g.lv.wrap_d[kk] = -(nrow[l] - 1) * pitch[l] * 128 - 2 * SUB * SUB_BYTES;
    lds += (size_t)nrow[l] * pitch[l] * 128;           // a multiple of 256: pitch is even
  }
  g.lds = lds;
  g.tiles.assign((size_t)g.ntiles, WinTile());
  g.pieces.assign((size_t)g.ntiles * 2 * G::NW * G::PCAP, typename G::Piece());
  g.qtab.assign((size_t)g.ntiles * G::QCAP, 0);
  std::vector<int> n_enter((size_t)g.ntiles, 0);
  for (int tx = 0; tx < tiles_x; ++tx)
    for (int ty = 0; ty < tiles_y; ++ty) {
      const size_t tile = (size_t)tx * tiles_y + ty;
      int pre[UNIVS_MAX_LEVELS + 1] = {0};
      for (int l = 0; l < L; ++l) pre[l + 1] = pre[l] + ax[(size_t)l * tiles_x + tx].y * ay[(size_t)l * tiles_y + ty].y;
      g.qmax = std::max<long long>(g.qmax, pre[L]);
      if (pre[L] >= 1 && pre[L] <= G::QCAP) {
        int last = 0;
        for (int l = 0; l < L; ++l) {
          const int4 gx = ax[(size_t)l * tiles_x + tx], gy = ay[(size_t)l * tiles_y + ty];
          for (int i = 0; i < gx.y * gy.y; ++i)
            g.qtab[tile * G::QCAP + pre[l] + i] = last = lv.start[l] + (gy.x + i / gx.y) * lv.W[l] + gx.x + i % gx.y;
        }
        for (int i = pre[L]; i < G::QCAP; ++i) g.qtab[tile * G::QCAP + i] = last;
      } else {
        g.ok = false;
      }
      WinTile& t = g.tiles[tile];
      std::memset(&t, 0, sizeof(t));
      t.total = pre[L];
      for (int which = 0; which < 2; ++which) {   // 0: entering rows, 1: whole windows
        int count = 0;
        for (int kk = 0; kk < L; ++kk) {
          const int l = ord[kk];
          const int4 gx = ax[(size_t)l * tiles_x + tx], gy = ay[(size_t)l * tiles_y + ty];
          if (gx.z + 1 < 0 || gx.z + 1 > 0xfff || gy.z + 1 < 0 || gy.z + 1 > 0xfff || nrow[l] > 63 || gx.w < 2 || gy.w < 2 ||
              gx.w - 2 > 0xff || gy.w - 2 > 0xff) g.ok = false;
          t.p0[kk] = (unsigned)(gx.z + 1) | ((unsigned)(gy.z + 1) << 12) |
                     ((unsigned)win_pos_mod((gy.z + 1) >> G::ROW_SHIFT, nrow[l]) << 24) | ((unsigned)((gy.z + 1) & SUB) << 30);
          t.p1[kk] = (unsigned)(gx.w - 2) | ((unsigned)(gy.w - 2) << 8);
          if (gy.z < -1 || gx.z < -1) g.ok = false;   // (axis_entry clips windows to the zero ring)
          int y0 = gy.z, n = gy.w;
          if (which == 0 && ty > 0) {
            const int4 py = ay[(size_t)l * tiles_y + ty - 1];
            if (G::MONOTONIC && gy.z < py.z) g.ok = false;
            y0 = std::max(gy.z, py.z + py.w);
            n = std::max(0, gy.z + gy.w - y0);
          }
          for (int r = 0; r < n; ++r) {
            const int y = y0 + r, Y = y + 1;
            const int lrow = win_pos_mod(Y >> G::ROW_SHIFT, nrow[l]);
            for (int b = 0; b * G::BLOCK < pitch[l]; ++b) {
              int px = lv.start[l] + y * lv.W[l] + gx.z + G::BLOCK * b;
              const int ldsoff = g.lv.reg[kk] + (lrow * pitch[l] + G::BLOCK * b) * 128 + (Y & SUB) * SUB_BYTES;
              unsigned ldmask = 0, stmask = 0;   // columns inside the level (load) / inside the window pitch (store)
              for (int i = 0; i < G::BLOCK; ++i) {
                const int cx = G::BLOCK * b + i, x = gx.z + cx;
                if (cx < pitch[l]) stmask |= 1u << i;
                if (cx < pitch[l] && y >= 0 && y < lv.H[l] && x >= 0 && x < lv.W[l]) ldmask |= 1u << i;
              }
              px = ldmask ? px + G::PX_BIAS : 0;
              if (px < 0 || px >= (1 << 24) || ldsoff >= (1 << 20)) g.ok = false;
              const int w = count % G::NW, j = count / G::NW;
              if (j < G::PCAP) g.pieces[((tile * 2 + which) * G::NW + w) * G::PCAP + j] = G::pack((unsigned)px & 0xffffffu, (unsigned)ldsoff, ldmask, stmask, kk);
              else g.ok = false;
              ++count;
            }
          }
        }
        const int per_wave = (count + G::NW - 1) / G::NW;
        if (which == 0) n_enter[tile] = per_wave;
        else t.n_cold = per_wave;
      }
    }
  for (size_t tile = 0; tile < (size_t)g.ntiles; ++tile) g.tiles[tile].n_enter = n_enter[(tile + (G::ENTER_OF_NEXT ? 1 : 0)) % g.ntiles];
  if (g.qmax < 1 || g.qmax > G::QCAP) g.ok = false;
  return g.ok;
}

}  // namespace univs
