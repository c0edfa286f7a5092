// Host-side tables of the "strips" MSDA kernel (msda_strips.hip, generation 5): pure C++ (no HIP calls), so that the
// host emulator (tools/strips_emulate.cpp) builds the very tables the kernel reads.
//
// Tiles, windows, the tile header, the host container and the table builder: msda_window_geom.h.  Here: this generation's
// constants, its traits for the builder (S5Geom), its level / piece structs and its sample record.
//
// LDS layout (one region per level).  A workgroup handles HALF a head (16 channels = 64 bytes per pixel).  A 128-byte
// LDS "super-pixel" holds pixel x of TWO consecutive level rows: with Y = y + 1 >= 0 (row -1 is the zero ring),
//     byte address = region + (((Y >> 1) mod NSR) * pitch + (x - wx0)) * 128 + (Y & 1) * 64 + chunk * 16.
// Rows are circular over the NSR super-rows: moving one tile down replaces only the rows that left the window.  The row
// below a sample's top row is at +64 (same super-row) or in the next super-row, which wraps to super-row 0 (no mirror
// row: it would cost 8 KB of the 80 KB a workgroup may use).  The four 16-byte chunk slots x {x parity} x {row parity} of a
// bilinear footprint are the 16 slots of the 256-byte LDS bank row: a lane visits its four corners and four chunks in a
// lane-specific order (msda_strips.hip) and the 16 lanes of a ds_read_b128 group never share a slot.  `pitch` is even
// (the x parity of the lower corners then equals that of the upper ones).
#pragma once
#include "msda_window_geom.h"

namespace univs {

constexpr int S5_NW = 8;             // waves of a workgroup; wave w owns the queries [16 w, 16 w + 16) of an item
constexpr int S5_QCAP = 16 * S5_NW;
constexpr int S5_PC = 4;             // row pieces a wave stages in registers per pass
constexpr int S5_PCAP = 32;          // row pieces per wave and list (<= 64: a wave fetches its list with one load)
constexpr int S5_ROWS_MAX = 26, S5_PITCH_MAX = 32;   // window caps (rows, pixels)
constexpr int S5_PX_BIAS = 16;
constexpr int S5_LMAX = WIN_LMAX;
constexpr int S5_DH = 16;            // channels per pass (half a head)
constexpr int S5_LDS_MAX = 80 * 1024;   // two workgroups per CU

// Per level slot (visiting order: largest level first), the same for every tile: a kernel argument.
struct S5Levels {
  int H[S5_LMAX], W[S5_LMAX], start[S5_LMAX], l[S5_LMAX];
  int pitch[S5_LMAX], reg[S5_LMAX], nsr[S5_LMAX];   // LDS row pitch (pixels, even), region byte offset, super-rows
  float rW[S5_LMAX], rH[S5_LMAX];                   // 1 / W, 1 / H correctly rounded (exact division by two FMAs)
  int next_d[S5_LMAX], wrap_d[S5_LMAX];             // byte distance from a sample's top row in the ODD half of a super-row to
                                                    // the row below it, minus 64: pitch * 128 - 128, and the same when the
                                                    // next super-row wraps to super-row 0: -(nsr - 1) * pitch * 128 - 128
};
// Per tile: WinTile, n_enter = pieces per wave of the NEXT tile's "entering rows" list (next in the sequence, wrapping);
// in p0, rot = ((wy0 + 1) >> 1) mod nsr = LDS super-row of the window's first row, par = (wy0 + 1) & 1 = the half of that
// super-row it lives in.
using S5Tile = WinTile;
__host__ __device__ __forceinline__ int s5_par(unsigned p0) { return (int)((p0 >> 30) & 1u); }
// One (row, 16-pixel column block) of one level's window: what one wave instruction moves (4 lanes x 16 B per pixel).
struct S5Piece {
  unsigned a;   // S5_PX_BIAS + pixel index (start + y * W + x) of the block's first pixel within the frame (24 bits) |
                // level slot << 24
  unsigned b;   // byte offset of the block's first pixel in LDS (row half included)
  unsigned c;   // columns inside the level (load mask, 16 bits) | columns inside the window pitch (store mask) << 16
  unsigned d;   // 0
};

// ---- a lane's sample record at one level (WinRec): shared by the kernel and the host emulator (tools/strips_emulate.cpp).
// Inputs: the sample's normalised location (x, y) and attention weight (FINITE: like the split-bf16 Linears that produce
// them, this path does not define results for inf / NaN activations), the level's size as floats, the tile's packed window
// words p0 / p1 (S5Tile), the level's nsr / pitch / next_d / wrap_d and the byte address of its LDS region, and the lane's
// low four bits.  The chunk rotation is in bits 4-5 of the addresses.
using S5Rec = WinRec;
__host__ __device__ __forceinline__ S5Rec s5_record(float x, float y, float awt, float Hf, float Wf, unsigned p0, unsigned p1,
                                                    int nsr, int pitch, int next_d, int wrap_d, unsigned region, unsigned lane4) {
  // reference arithmetic: ms_deform_im2col_cuda.cuh:285-293 and :38-89; the window includes the one-pixel zero ring around
  // the level, so out-of-level corners simply read zeros
  const float him = fmaf(y, Hf, -0.5f), wim = fmaf(x, Wf, -0.5f);
  const int r0 = win_floor_to_int(him) - win_wy0(p0), c0 = win_floor_to_int(wim) - win_wx0(p0);
  const float lh = win_fract(him), lw = win_fract(wim);
  // Footprint inside the window?  A window never leaves the ring-extended level, so an in-window sample is inside the
  // reference's band (-1, H) x (-1, W) -- except exactly on its open edge (him == -1), where the bilinear weights of the
  // only in-level row are 0 anyway: the band test of cuh:293 is implied.
  S5Rec rec;
  rec.inwin = (unsigned)r0 <= ((p1 >> 8) & 0xffu) && (unsigned)c0 <= (p1 & 0xffu);
  // (a sample that must not contribute still reads: everything is masked to the window's first pixel, which is always
  // staged; its attention weight becomes an exact 0)
  const unsigned m = rec.inwin ? 0xffffffffu : 0u;
  const float aw = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, awt) & m);
  // window row r0 -> (super-row, half): rows are paired by the parity of y + 1
  const unsigned yrel = ((unsigned)r0 & m) + (unsigned)s5_par(p0);
  const unsigned hy = yrel & 1u;
  unsigned srl = (yrel >> 1) + (unsigned)win_rot(p0);
  const unsigned srw = srl - (unsigned)nsr;
  srl = srl < srw ? srl : srw;                   // circular: srl - nsr underflows to a huge number unless srl >= nsr
  const unsigned idx = win_mul24(srl, (unsigned)pitch) + ((unsigned)c0 & m);
  const unsigned r4 = ((lane4 >> 2) & 3u) << 4;
  const unsigned tl = ((idx << 7) + region) | (hy << 6) | r4;
  // the row below: the other half of the same super-pixel (+64), or the first half of the next super-row (circular)
  const int nd = (srl + 1u == (unsigned)nsr) ? wrap_d : next_d;
  const unsigned below = 64u + ((unsigned)nd & (0u - hy));
  const unsigned lb0 = lane4 & 1u, lb1 = (lane4 >> 1) & 1u;
  const unsigned fs = ((tl >> 7) ^ lb0) & 1u;   // which corner column I read first
  const unsigned ft = hy ^ lb1;                 // which corner row I read first
  const unsigned c00 = tl + (fs << 7), c01 = tl + ((fs ^ 1u) << 7);
  const unsigned rowd = below & (0u - ft), rowd2 = below - rowd;
  rec.a[0] = c00 + rowd; rec.a[1] = c01 + rowd; rec.a[2] = c00 + rowd2; rec.a[3] = c01 + rowd2;
  const float f0 = fs ? lw : 1.f - lw;          // column weight of the corner column read first
  const float g0 = ft ? lh : 1.f - lh;          // row weight of the corner row read first
  const float wr0 = aw * g0, wr1 = aw - wr0;
  rec.w[0] = wr0 * f0; rec.w[1] = wr0 - rec.w[0]; rec.w[2] = wr1 * f0; rec.w[3] = wr1 - rec.w[2];
  return rec;
}
// ---- what the shared table builder (msda_window_geom.h: win_build_host) needs to know about this generation
struct S5Geom {
  using Levels = S5Levels;
  using Piece = S5Piece;
  static constexpr int (S5Levels::*ROWS)[S5_LMAX] = &S5Levels::nsr;
  static constexpr int NW = S5_NW, QCAP = S5_QCAP, PCAP = S5_PCAP, ROWS_MAX = S5_ROWS_MAX, PITCH_MAX = S5_PITCH_MAX;
  static constexpr int BLOCK = 16, PX_BIAS = S5_PX_BIAS;
  static constexpr int ROW_SHIFT = 1;              // super-rows: two level rows per LDS row, 64 bytes per pixel each
  static constexpr bool ENTER_OF_NEXT = true;      // the kernel fetches the next tile's entering rows with this tile's header
  static constexpr bool MONOTONIC = false;
  static S5Piece pack(unsigned px, unsigned ldsoff, unsigned ldmask, unsigned stmask, int slot) {
    return S5Piece{px | ((unsigned)slot << 24), ldsoff, ldmask | (stmask << 16), 0u};
  }
};
using S5Host = WinHost<S5Geom>;
static inline bool s5_build_host(const LevelTable& lv, int L, int fine, int TH, int TW, int R, S5Host& g) {
  return win_build_host<S5Geom>(lv, L, fine, TH, TW, R, g);
}

}  // namespace univs
