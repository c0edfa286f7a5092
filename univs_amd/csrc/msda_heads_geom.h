// Host-side tables of the "heads" MSDA kernel (msda_heads.hip, generation 6): pure C++ (no HIP calls), so that the host
// emulator (tools/heads_emulate.cpp) builds the very tables the kernel reads.
//
// Tiles, windows, the tile header, the host container and the table builder: msda_window_geom.h.  Here: this generation's
// constants, its traits for the builder (S6Geom), its level / piece structs, its sample record and the segment builder: a
// workgroup walks down SEGMENTS of tile columns (S6Seg: plane = (frame, head), first tile, count).
//
// LDS layout (one region per level).  A workgroup handles a FULL head: 32 channels = 128 bytes per pixel = half a 256-byte
// LDS bank row.  With Y = y + 1 >= 0 (row -1 is the zero ring) and rows circular over the level's NR window rows,
//     byte address = region + ((Y mod NR) * pitch + (x - wx0)) * 128 + chunk * 16          (pitch even, region % 256 == 0)
// so bit 7 of a pixel's address is the parity of its window column.  The 16 lanes of a ds_read_b128 group have 16
// different low-four lane bits (MI355X_MICROARCH.md, LDS table): a lane reads the horizontal corner whose column parity
// equals its lane bit 3 first, and the eight 16-byte chunks of a pixel in the order j ^ (lane & 7): the 16 lanes of a group
// hit 16 different 16-byte slots of the 256-byte bank row whatever pixels they sample -- conflict-free by construction.
#pragma once
#include "msda_window_geom.h"

namespace univs {

constexpr int S6_NW = 8;             // waves of a workgroup; wave w owns the queries [16 w, 16 w + 16) of an item
constexpr int S6_QCAP = 16 * S6_NW;  // queries per item
constexpr int S6_PC = 8;             // row pieces a wave stages in registers per pass
constexpr int S6_PCAP = 32;          // row pieces per wave and list (<= 64: a wave fetches its list with one load)
constexpr int S6_ROWS_MAX = 40, S6_PITCH_MAX = 48;   // window caps (rows, pixels)
constexpr int S6_PX_BIAS = 8;
constexpr int S6_LMAX = WIN_LMAX;
constexpr int S6_DH = 32;            // channels per lane-sample (a full head)
constexpr int S6_LDS_MAX = 160 * 1024;   // one workgroup per CU

// Per level slot (visiting order: largest level first), the same for every tile: a kernel argument.
struct S6Levels {
  int H[S6_LMAX], W[S6_LMAX], start[S6_LMAX], l[S6_LMAX];
  int pitch[S6_LMAX], reg[S6_LMAX], nr[S6_LMAX];   // LDS row pitch (pixels, even), region byte offset, circular rows
  float rW[S6_LMAX], rH[S6_LMAX];                  // 1 / W, 1 / H correctly rounded (exact division by two FMAs)
  int next_d[S6_LMAX], wrap_d[S6_LMAX];            // byte distance from a row to the row below it: pitch * 128, and the same
                                                   // when the row below wraps to row 0: -(nr - 1) * pitch * 128
};
// Per tile: WinTile, n_enter = pieces per wave of this tile's own "entering rows" list; in p0, rot = (wy0 + 1) mod nr = LDS
// row of the window's first row (par = 0).
using S6Tile = WinTile;
// One (row, 8-pixel column block) of one level's window: what one wave instruction moves (8 lanes x 16 B per pixel).
struct S6Piece {
  unsigned a;   // S6_PX_BIAS + pixel index (start + y * W + x) of the block's first pixel within the frame (24 bits) |
                // columns inside the level (load mask, 8 bits) << 24
  unsigned b;   // byte offset of the block's first pixel in LDS (24 bits) | columns inside the window pitch (store mask) << 24
};
// A workgroup's work: `count` consecutive tiles of one column of one (frame, head) plane, first tile `tile0`.
struct S6Seg {
  int plane, tile0, count, pad;
};

// ---- a lane's sample record at one level (WinRec): shared by the kernel and the host emulator (tools/heads_emulate.cpp).
// Inputs: the sample's normalised location (x, y) and attention weight (FINITE), the level's size as floats, the tile's
// packed window words p0 / p1 (S6Tile), the level's nr / pitch / next_d / wrap_d, the byte address of its LDS region and the
// lane's low four bits.  The corners come in the order first / second horizontal corner of the top row, then of the bottom
// row; the lane's chunk rotation is in bits 4-6 of the addresses.
using S6Rec = WinRec;
__host__ __device__ __forceinline__ S6Rec s6_record(float x, float y, float awt, float Hf, float Wf, unsigned p0, unsigned p1,
                                                    int nr, int pitch, int next_d, int wrap_d, unsigned region, unsigned lane4) {
  // reference arithmetic: ms_deform_im2col_cuda.cuh:285-293 and :38-89; the window includes the one-pixel zero ring around
  // the level, so out-of-level corners simply read zeros
  const float him = fmaf(y, Hf, -0.5f), wim = fmaf(x, Wf, -0.5f);
  const int r0 = win_floor_to_int(him) - win_wy0(p0), c0 = win_floor_to_int(wim) - win_wx0(p0);
  const float lh = win_fract(him), lw = win_fract(wim);
  // Footprint inside the window?  A window never leaves the ring-extended level, so an in-window sample is inside the
  // reference's band (-1, H) x (-1, W) -- except exactly on its open edge (him == -1), where the bilinear weights of the
  // only in-level row are 0 anyway: the band test of cuh:293 is implied.
  S6Rec rec;
  rec.inwin = (unsigned)r0 <= ((p1 >> 8) & 0xffu) && (unsigned)c0 <= (p1 & 0xffu);
  // (a sample that must not contribute still reads: everything is masked to the window's first pixel, which is always
  // staged; its attention weight becomes an exact 0)
  const unsigned m = rec.inwin ? 0xffffffffu : 0u;
  const float aw = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, awt) & m);
  const unsigned cm = (unsigned)c0 & m;
  unsigned row = ((unsigned)r0 & m) + (unsigned)win_rot(p0);
  const unsigned roww = row - (unsigned)nr;
  row = row < roww ? row : roww;                 // circular: row - nr underflows to a huge number unless row >= nr
  const unsigned idx = win_mul24(row, (unsigned)pitch) + cm;
  const unsigned fs = (cm ^ (lane4 >> 3)) & 1u;  // 1: the RIGHT corner's column parity equals my lane bit 3 -> I read it first
  const unsigned base = (idx << 7) + region + ((lane4 & 7u) << 4);
  const unsigned first = base + (fs << 7), second = base + ((fs ^ 1u) << 7);
  const unsigned nd = (unsigned)((row + 1u == (unsigned)nr) ? wrap_d : next_d);
  rec.a[0] = first; rec.a[1] = second; rec.a[2] = first + nd; rec.a[3] = second + nd;
  const float f0 = fs ? lw : 1.f - lw;           // column weight of the corner column read first
  const float wb = aw * lh, wt = aw - wb;        // row weights: bottom, top
  rec.w[0] = wt * f0; rec.w[1] = wt - rec.w[0]; rec.w[2] = wb * f0; rec.w[3] = wb - rec.w[2];
  return rec;
}
// ---- what the shared table builder (msda_window_geom.h: win_build_host) needs to know about this generation
struct S6Geom {
  using Levels = S6Levels;
  using Piece = S6Piece;
  static constexpr int (S6Levels::*ROWS)[S6_LMAX] = &S6Levels::nr;
  static constexpr int NW = S6_NW, QCAP = S6_QCAP, PCAP = S6_PCAP, ROWS_MAX = S6_ROWS_MAX, PITCH_MAX = S6_PITCH_MAX;
  static constexpr int BLOCK = 8, PX_BIAS = S6_PX_BIAS;
  static constexpr int ROW_SHIFT = 0;              // a level row has an LDS row to itself: 128 bytes per pixel
  static constexpr bool ENTER_OF_NEXT = false;     // a segment may start at any tile: every tile's header counts its own rows
  static constexpr bool MONOTONIC = true;          // the entering rows of a tile assume that its windows start no higher than
                                                   // those of the tile above it
  static S6Piece pack(unsigned px, unsigned ldsoff, unsigned ldmask, unsigned stmask, int /*slot*/) {
    return S6Piece{px | (ldmask << 24), ldsoff | (stmask << 24)};
  }
};
using S6Host = WinHost<S6Geom>;
static inline bool s6_build_host(const LevelTable& lv, int L, int fine, int TH, int TW, int R, S6Host& g) {
  return win_build_host<S6Geom>(lv, L, fine, TH, TW, R, g);
}

// ---- who does what: `grid` workgroups, each a list of segments (workgroup b: segs[begin[b]] .. segs[begin[b + 1] - 1]), for
// `planes` (frame, head) planes of tiles_x columns of tiles_y tiles.  Workgroup b runs on XCD b % 8 (MI355X_MICROARCH.md: observed,
// used for speed only).
//   policy 0 -- contiguous ranges: the (plane, column, row) sequence is cut into `grid` equal ranges, the workgroups of an XCD
//     own neighbouring ranges (generation 5's rule).  Balanced to one tile, but two workgroups that work on horizontally
//     adjacent tiles do so at different times: each fetches its own halo columns from HBM.
//   policy 1 -- lockstep rounds: every XCD owns a contiguous eighth of the sequence and its W = grid / 8 workgroups walk W
//     ADJACENT columns top to bottom at the same time, round after round, so that the halo columns two neighbours share are
//     fetched from HBM once and found in that XCD's L2 by the other; the columns left over after the last full round are cut
//     into equal pieces or equal ranges, whichever estimates the smaller makespan (a cold start priced at `cold_steps` tiles).
static bool s6_build_segments_lists(int planes, int tiles_x, int tiles_y, int grid, int policy, double cold_steps,
                                    std::vector<std::vector<S6Seg>>& lists) {
  lists.assign((size_t)std::max(grid, 0), std::vector<S6Seg>());
  const long long ncol = (long long)planes * tiles_x, total = ncol * tiles_y;
  if (grid < 1 || total < 1) return false;
  auto push = [&](int wg, long long col, int y0, int n) -> bool {   // rows [y0, y0 + n) of linear column `col`
    if (n <= 0) return true;
    const int plane = (int)(col / tiles_x), tx = (int)(col % tiles_x);
    lists[(size_t)wg].push_back(S6Seg{plane, tx * tiles_y + y0, n, 0});
    return true;
  };
  auto range = [&](int wg, long long g0, long long g1) -> bool {   // the steps [g0, g1) of the sequence, cut at column ends
    while (g0 < g1) {
      const long long col = g0 / tiles_y;
      const int y0 = (int)(g0 % tiles_y), n = (int)std::min<long long>(g1 - g0, tiles_y - y0);
      if (!push(wg, col, y0, n)) return false;
      g0 += n;
    }
    return true;
  };
  const int nx = 8;
  if (policy == 0 || grid % nx != 0 || grid / nx < 2) {
    const int gq = grid / std::min(nx, grid), gr = grid % std::min(nx, grid), nxe = std::min(nx, grid);
    for (int b = 0; b < grid; ++b) {
      const int xcd = b % nxe, widx = b / nxe;
      const long long lw = (long long)xcd * gq + std::min(xcd, gr) + widx;
      if (!range(b, lw * total / grid, (lw + 1) * total / grid)) return false;
    }
    return true;
  }
  const int W = grid / nx;
  for (int x = 0; x < nx; ++x) {
    const long long s0 = (long long)x * total / nx, s1 = (long long)(x + 1) * total / nx;
    if (s0 >= s1) continue;
    struct Col { long long col; int y0, n; };
    std::vector<Col> cols;
    for (long long g0 = s0; g0 < s1;) {
      const int y0 = (int)(g0 % tiles_y), n = (int)std::min<long long>(s1 - g0, tiles_y - y0);
      cols.push_back(Col{g0 / tiles_y, y0, n});
      g0 += n;
    }
    const size_t full = cols.size() / W * W;
    for (size_t i = 0; i < full; ++i)
      if (!push((int)(x + nx * (i % W)), cols[i].col, cols[i].y0, cols[i].n)) return false;
    const size_t rem = cols.size() - full;
    if (!rem) continue;
    // The columns left over after the last full round, two ways; the smaller estimated makespan (tiles + `cold_steps` per
    // segment) wins:
    //  (a) every column cut into V equal pieces (V in 1..4), dealt longest-first: one segment per piece;
    //  (b) their tiles in sequence order cut into W equal ranges: balanced to one tile whatever the column count, a range that
    //      crosses a column end is two segments.
    struct Pc { long long col; int y0, n, wg; };
    auto plan_a = [&](int V, std::vector<Pc>& pcs) -> double {
      pcs.clear();
      for (size_t i = full; i < cols.size(); ++i)
        for (int v = 0; v < V; ++v) {
          const int a = cols[i].n * v / V, b = cols[i].n * (v + 1) / V;
          if (b > a) pcs.push_back(Pc{cols[i].col, cols[i].y0 + a, b - a, 0});
        }
      std::stable_sort(pcs.begin(), pcs.end(), [](const Pc& a, const Pc& b) { return a.n > b.n; });
      std::vector<double> load((size_t)W, 0.0);
      for (Pc& p : pcs) {
        p.wg = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        load[p.wg] += p.n + cold_steps;
      }
      return *std::max_element(load.begin(), load.end());
    };
    auto plan_b = [&](std::vector<Pc>& pcs) -> double {
      pcs.clear();
      long long rtot = 0;
      for (size_t i = full; i < cols.size(); ++i) rtot += cols[i].n;
      size_t ci = full;
      int used = 0;   // tiles of cols[ci] already dealt
      std::vector<double> load((size_t)W, 0.0);
      for (int j = 0; j < W; ++j) {
        long long want = rtot * (j + 1) / W - rtot * j / W;
        while (want > 0 && ci < cols.size()) {
          const int n = (int)std::min<long long>(want, cols[ci].n - used);
          pcs.push_back(Pc{cols[ci].col, cols[ci].y0 + used, n, j});
          load[j] += n + cold_steps;
          used += n;
          want -= n;
          if (used == cols[ci].n) { ++ci; used = 0; }
        }
      }
      return *std::max_element(load.begin(), load.end());
    };
    std::vector<Pc> best, cand;
    double bestms = plan_b(best);
    for (int V = 1; V <= 4; ++V) {
      const double ms = plan_a(V, cand);
      if (ms < bestms - 1e-9) { bestms = ms; best.swap(cand); }
    }
    for (const Pc& p : best)
      if (!push(x + nx * p.wg, p.col, p.y0, p.n)) return false;
  }
  return true;
}
static bool s6_build_segments(int planes, int tiles_x, int tiles_y, int grid, int policy, double cold_steps, std::vector<S6Seg>& segs,
                              std::vector<int>& begin) {
  std::vector<std::vector<S6Seg>> lists;
  segs.clear();
  begin.assign((size_t)std::max(grid, 0) + 1, 0);
  if (!s6_build_segments_lists(planes, tiles_x, tiles_y, grid, policy, cold_steps, lists)) return false;
  for (int b = 0; b < grid; ++b) {
    begin[b] = (int)segs.size();
    segs.insert(segs.end(), lists[b].begin(), lists[b].end());
  }
  begin[grid] = (int)segs.size();
  if (segs.empty()) segs.push_back(S6Seg{0, 0, 0, 0});   // (never read: keeps the upload non-empty)
  return true;
}

}  // namespace univs
