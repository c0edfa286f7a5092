// Polygons to run-length boundaries (include/univs_polygons_hip.h), as plain C++ for the host and the device: the rule of
// univs_amd/data/polygon_rule.py per point and per crossing, and the whole per-object schedule of csrc/polygon_runs.hip.  The
// lane-parallel half is the template parameter `Ex`:
//
//   ex.each(f)    runs f(tid) for every tid in [0, PG_THREADS), then orders all their stores before whatever follows
//                 (the device: f(threadIdx.x) and a barrier; tools/polygon_host.cpp: a loop over tid)
//   ex.read(p)    *p as a value all lanes agree on, safe against a later each() that rewrites it (the device: load, barrier)
//
// One workgroup takes one object.  Per polygon: the scaled vertices and the per-edge point counts go to LDS and are scanned; lanes stride
// over the polygon's global point index, find the edge by binary search and recompute the point and its predecessor; crossings are
// appended to the LDS keys and the polygon's segment is sorted.  A crossing of even rank in its polygon opens coverage (+1), one of odd
// rank closes it (-1): two crossings at one position cancel, which is the rule's parity.  All events of the object are sorted by
// position, summed by a scan, and a boundary is written wherever coverage passes between 0 and positive: the union of the polygons.
//
// The rules this file keeps for untrusted tables and coordinates:
//   * every table entry (obj_start, poly_start, slot, size) is clamped into its array before it indexes anything;
//   * every loop is counted by a clamped number: polygons of the object, PG_MAX_VERTS vertices, PG_MAX_POINTS points, PG_MAX_KEYS keys;
//   * every store to bounds / ones is checked against the object's own slots; a key is stored only below PG_MAX_KEYS;
//   * a coordinate that is not finite or beyond +-2^24 ends the object with PG_ST_MALFORMED before it is converted.
// The arithmetic is float64 in the order written; the file is compiled without contraction to fma (a fused ys + s t changes
// int(... + 0.5) at ties).
#ifndef UNIVS_POLYGON_CORE_H
#define UNIVS_POLYGON_CORE_H

#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PG_HD __host__ __device__ inline
#else
#define PG_HD inline
#endif

namespace univs {

// status[o] of univs_polygons_to_runs (include/univs_polygons_hip.h documents the values; tests pin them)
enum PgStatus {
  PG_ST_OK = 0,
  PG_ST_CROSSINGS = 1,   // more than PG_MAX_KEYS crossings
  PG_ST_POINTS = 2,      // a polygon of more than PG_MAX_POINTS points
  PG_ST_SIZE = 3,        // h < 1, w < 1 or h w >= 2^31
  PG_ST_VERTICES = 4,    // a polygon of more than PG_MAX_VERTS vertices
  PG_ST_MALFORMED = 5,   // a polygon of fewer than 3 points, a coordinate that is not finite or beyond +-2^24
  PG_ST_SLOTS = 6        // the object's slots are too few for its boundaries
};

constexpr int PG_THREADS = 256;
constexpr int PG_MAX_KEYS = 16384;           // crossings of one object: 64 KB of LDS keys
constexpr int PG_MAX_VERTS = 4096;           // vertices of one polygon: 48 KB of LDS (X, Y, the scanned point counts)
constexpr int PG_MAX_POINTS = 1 << 22;       // points of one polygon
constexpr double PG_COORD_LIMIT = 16777216.0;
constexpr unsigned PG_DROPPED = 0xFFFFFFFFu;  // a key at h w: not a boundary, sorted behind all others

struct PgArgs {
  const double* xy;            // [2 n_points]
  const int* poly_start;       // [P + 1], in points
  const int* obj_start;        // [N + 1], in polygons
  const int* size;             // [N, 2]: h, w
  const long long* slot;       // [N + 1]: the object's slots are slot[o] .. slot[o + 1] of bounds / ones
  int* bounds;
  int* ones;
  int* count;                  // [N]
  int* status;                 // [N]
  long long n_points, cap_total;
  int P, N;
};

// the workgroup's LDS (the host tool: heap blocks of exactly these sizes)
struct PgLds {
  int* X;                      // [PG_MAX_VERTS + 1]
  int* Y;                      // [PG_MAX_VERTS + 1]
  int* off;                    // [PG_MAX_VERTS + 1]: points before edge e; off[nv] = the polygon's points
  unsigned* keys;              // [PG_MAX_KEYS]
  int* part;                   // [PG_THREADS + 1]
  int* part2;                  // [PG_THREADS + 1]
  unsigned long long* flags;   // [PG_THREADS]
  int* ctr;                    // [4]: keys appended, keys dropped, a bad coordinate was seen, (free)
  unsigned short* cover;       // [PG_MAX_KEYS]: coverage after key i
};
constexpr int PG_LDS_INTS = 3 * (PG_MAX_VERTS + 1);

PG_HD int pg_clampi(long long v, long long lo, long long hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }
PG_HD long long pg_clampl(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

PG_HD bool pg_coord_ok(double x) { return x >= -PG_COORD_LIMIT && x <= PG_COORD_LIMIT; }   // (false for a NaN)

// step 1: int(5 x + 0.5), C's conversion; x has passed pg_coord_ok
PG_HD int pg_scale(double x) { return (int)(5.0 * x + 0.5); }

PG_HD int pg_abs(int v) { return v < 0 ? -v : v; }

// step 2: the points of edge e
PG_HD int pg_edge_points(const int* X, const int* Y, int e) {
  const int dx = pg_abs(X[e + 1] - X[e]), dy = pg_abs(Y[e + 1] - Y[e]);
  return (dx >= dy ? dx : dy) + 1;
}

// step 2: point d (from the edge's original start) of edge e
PG_HD void pg_point(const int* X, const int* Y, int e, int d, int* u, int* v) {
  int xs = X[e], xe = X[e + 1], ys = Y[e], ye = Y[e + 1];
  const int dx = pg_abs(xe - xs), dy = pg_abs(ye - ys);
  const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
  if (flip) {
    int t = xs;
    xs = xe, xe = t;
    t = ys, ys = ye, ye = t;
  }
  if (dx >= dy) {
    const double s = dx == 0 ? 0.0 : (double)(ye - ys) / (double)dx;
    const int t = flip ? dx - d : d;
    *u = t + xs;
    *v = (int)((double)ys + s * (double)t + 0.5);
  } else {
    const double s = (double)(xe - xs) / (double)dy;
    const int t = flip ? dy - d : d;
    *v = t + ys;
    *u = (int)((double)xs + s * (double)t + 0.5);
  }
}

// step 3 between a point (u0, v0) and its successor (u1, v1), in integers: the column exists exactly where the smaller side is
// 2 (mod 5), the row is ceil((vmin - 2) / 5) clamped to [0, h]
PG_HD bool pg_crossing(int u0, int v0, int u1, int v1, int h, int w, unsigned* pos) {
  if (u1 == u0) return false;
  const int ms = u1 < u0 ? u1 : u1 - 1;
  if (ms < 2 || (ms - 2) % 5 != 0) return false;           // (a column below 0 is outside the image)
  const int col = (ms - 2) / 5;
  if (col > w - 1) return false;
  const int a = (v0 < v1 ? v0 : v1) - 2;
  int row = a >= 0 ? (a + 4) / 5 : -((-a) / 5);
  row = row < 0 ? 0 : (row > h ? h : row);
  *pos = (unsigned)col * (unsigned)h + (unsigned)row;      // <= h w < 2^31
  return true;
}

// the edge that holds global point g: the last e in [0, nv) with off[e] <= g (off[0] = 0, increasing)
PG_HD int pg_find_edge(const int* off, int nv, int g) {
  int lo = 0, hi = nv - 1;
  for (int it = 0; it < 13 && lo < hi; ++it) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= g)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// the first index in [0, n) whose position is >= pos (n where there is none); keys sorted by position
PG_HD int pg_first_at(const unsigned* keys, int n, unsigned pos) {
  int lo = 0, hi = n;
  for (int it = 0; it < 15 && lo < hi; ++it) {
    const int mid = (lo + hi) >> 1;
    if ((keys[mid] >> 1) < pos)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ascending sort of keys[0, n) by the workgroup: the bitonic network whose exchanges all put the smaller key at the lower index, so
// that the keys a power of two would add (all "larger than any") never move and are left out
template <class Ex>
PG_HD void pg_sort(Ex& ex, unsigned* keys, int n) {
  if (n > PG_MAX_KEYS) n = PG_MAX_KEYS;
  for (int size = 2; size < 2 * n; size <<= 1) {
    for (int j = size >> 1; j > 0; j >>= 1) {
      const int mask = j == (size >> 1) ? size - 1 : j;    // the first step of a merge mirrors, the others shift
      ex.each([&](int tid) {
        for (int i = tid; i < n; i += PG_THREADS) {
          const int l = i ^ mask;
          if (l > i && l < n) {
            const unsigned a = keys[i], b = keys[l];
            if (a > b) keys[i] = b, keys[l] = a;
          }
        }
      });
    }
  }
}

// part[0 .. PG_THREADS) -> its exclusive prefix sums, part[PG_THREADS] = the total, capped at `cap` (the sums of untrusted counts)
template <class Ex>
PG_HD void pg_scan(Ex& ex, int* part, int cap) {
  ex.each([&](int tid) {
    if (tid != 0) return;
    int run = 0;
    for (int t = 0; t < PG_THREADS; ++t) {
      const int v = part[t];
      part[t] = run;
      const long long s = (long long)run + v;
      run = s > cap ? cap : (s < -(long long)cap ? -cap : (int)s);
    }
    part[PG_THREADS] = run;
  });
}

template <class Ex>
PG_HD void pg_finish(Ex& ex, const PgArgs& A, int o, int status, int count) {
  ex.each([&](int tid) {
    if (tid == 0) A.status[o] = status, A.count[o] = count;
  });
}

// object o of the call, by the whole workgroup
template <class Ex>
PG_HD void pg_object(Ex& ex, const PgArgs& A, int o, const PgLds& L) {
  const int h = A.size[2 * (long long)o], w = A.size[2 * (long long)o + 1];
  const int p0 = pg_clampi(A.obj_start[o], 0, A.P), p1 = pg_clampi(A.obj_start[o + 1], p0, A.P);
  const long long s0 = pg_clampl(A.slot[o], 0, A.cap_total), s1 = pg_clampl(A.slot[o + 1], s0, A.cap_total);
  const long long cap = s1 - s0;
  if (p1 == p0) return pg_finish(ex, A, o, PG_ST_OK, 0);                       // absent: no boundary at all
  if (h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return pg_finish(ex, A, o, PG_ST_SIZE, 0);
  const unsigned hw = (unsigned)h * (unsigned)w;
  ex.each([&](int tid) {
    if (tid < 4) L.ctr[tid] = 0;
  });

  for (int p = p0; p < p1; ++p) {
    const long long a = pg_clampl(A.poly_start[p], 0, A.n_points), b = pg_clampl(A.poly_start[p + 1], a, A.n_points);
    if (b - a < 3) return pg_finish(ex, A, o, PG_ST_MALFORMED, 0);
    if (b - a > PG_MAX_VERTS) return pg_finish(ex, A, o, PG_ST_VERTICES, 0);
    const int nv = (int)(b - a);
    // step 1
    ex.each([&](int tid) {
      for (int i = tid; i < nv; i += PG_THREADS) {
        const double x = A.xy[2 * (a + i)], y = A.xy[2 * (a + i) + 1];
        const bool ok = pg_coord_ok(x) && pg_coord_ok(y);
        if (!ok) L.ctr[2] = 1;
        L.X[i] = ok ? pg_scale(x) : 0;
        L.Y[i] = ok ? pg_scale(y) : 0;
        if (i == 0) L.X[nv] = L.X[0], L.Y[nv] = L.Y[0];
      }
    });
    if (ex.read(&L.ctr[2])) return pg_finish(ex, A, o, PG_ST_MALFORMED, 0);
    // the points before every edge
    const int per = (nv + PG_THREADS - 1) / PG_THREADS;
    ex.each([&](int tid) {
      int sum = 0;
      for (int e = tid * per; e < nv && e < (tid + 1) * per; ++e) {
        sum += pg_edge_points(L.X, L.Y, e);
        if (sum > PG_MAX_POINTS + 1) sum = PG_MAX_POINTS + 1;
      }
      L.part[tid] = sum;
    });
    pg_scan(ex, L.part, PG_MAX_POINTS + 1);
    ex.each([&](int tid) {
      int run = L.part[tid];
      for (int e = tid * per; e < nv && e < (tid + 1) * per; ++e) {
        L.off[e] = run;
        run += pg_edge_points(L.X, L.Y, e);
        if (run > PG_MAX_POINTS + 1) run = PG_MAX_POINTS + 1;
      }
      if (tid == 0) L.off[nv] = L.part[PG_THREADS];
    });
    const int m = ex.read(&L.off[nv]);
    if (m > PG_MAX_POINTS) return pg_finish(ex, A, o, PG_ST_POINTS, 0);
    // steps 2 and 3: global point g against its predecessor
    const int base = ex.read(&L.ctr[0]);
    ex.each([&](int tid) {
      for (int g = 1 + tid; g < m; g += PG_THREADS) {
        const int e = pg_find_edge(L.off, nv, g);
        const int d = pg_clampi(g - L.off[e], 0, pg_edge_points(L.X, L.Y, e) - 1);
        int u1, v1, u0, v0;
        pg_point(L.X, L.Y, e, d, &u1, &v1);
        if (d > 0)
          pg_point(L.X, L.Y, e, d - 1, &u0, &v0);
        else if (e > 0)                                                              // (always, for g >= 1)
          pg_point(L.X, L.Y, e - 1, pg_edge_points(L.X, L.Y, e - 1) - 1, &u0, &v0);
        else
          continue;
        unsigned pos;
        if (pg_crossing(u0, v0, u1, v1, h, w, &pos)) {
          const int at = ex.append(&L.ctr[0]);
          if (at >= 0 && at < PG_MAX_KEYS) L.keys[at] = pos;
        }
      }
    });
    const int end = ex.read(&L.ctr[0]);
    if (end > PG_MAX_KEYS || end < base) return pg_finish(ex, A, o, PG_ST_CROSSINGS, 0);
    pg_sort(ex, L.keys + base, end - base);
    // a crossing of even rank opens, one of odd rank closes; at h w nothing is stored
    ex.each([&](int tid) {
      for (int i = base + tid; i < end; i += PG_THREADS) {
        const unsigned pos = L.keys[i];
        if (pos >= hw) {
          L.keys[i] = PG_DROPPED;
          ex.append(&L.ctr[1]);
        } else {
          L.keys[i] = (pos << 1) | (unsigned)((i - base) & 1);
        }
      }
    });
  }

  const int all = ex.read(&L.ctr[0]);
  const int n = all - pg_clampi(ex.read(&L.ctr[1]), 0, all);                     // the dropped keys are the last ones after the sort
  if (p1 - p0 > 1) pg_sort(ex, L.keys, all);
  // coverage after every key: +1 for an opening, -1 for a closing one
  const int per = (n + PG_THREADS - 1) / PG_THREADS;                            // <= 64: a lane's flags are one 64-bit word
  ex.each([&](int tid) {
    int sum = 0;
    for (int i = tid * per; i < n && i < (tid + 1) * per; ++i) sum += (L.keys[i] & 1u) ? -1 : 1;
    L.part[tid] = sum;
  });
  pg_scan(ex, L.part, PG_MAX_KEYS);
  ex.each([&](int tid) {
    int run = L.part[tid];
    for (int i = tid * per; i < n && i < (tid + 1) * per; ++i) {
      run += (L.keys[i] & 1u) ? -1 : 1;
      L.cover[i] = (unsigned short)(run < 0 ? 0 : run);
    }
  });
  // a boundary: the last key of a position, where coverage before the position's first key and after its last differ in being 0
  ex.each([&](int tid) {
    unsigned long long f = 0;
    int c = 0;
    for (int i = tid * per; i < n && i < (tid + 1) * per; ++i) {
      const unsigned pos = L.keys[i] >> 1;
      if (i + 1 < n && (L.keys[i + 1] >> 1) == pos) continue;
      const int first = pg_first_at(L.keys, n, pos);
      const int before = first > 0 ? L.cover[first - 1] : 0, after = L.cover[i];
      if ((before > 0) != (after > 0)) f |= 1ull << (i - tid * per), ++c;
    }
    L.flags[tid] = f;
    L.part[tid] = c;
  });
  pg_scan(ex, L.part, PG_MAX_KEYS + 1);
  // ones[k]: boundary k closes a foreground run where k is odd -- an alternating sum of the positions
  ex.each([&](int tid) {
    const unsigned long long f = L.flags[tid];
    int k = L.part[tid], acc = 0;
    for (int i = tid * per; i < n && i < (tid + 1) * per; ++i)
      if ((f >> (i - tid * per)) & 1ull) acc += (k++ & 1) ? (int)(L.keys[i] >> 1) : -(int)(L.keys[i] >> 1);
    L.part2[tid] = acc;
  });
  pg_scan(ex, L.part2, 0x7FFFFFFF);
  ex.each([&](int tid) {
    const unsigned long long f = L.flags[tid];
    int k = L.part[tid], acc = L.part2[tid];
    for (int i = tid * per; i < n && i < (tid + 1) * per; ++i) {
      if (!((f >> (i - tid * per)) & 1ull)) continue;
      const int pos = (int)(L.keys[i] >> 1);
      acc += (k & 1) ? pos : -pos;
      if (k < cap) A.bounds[s0 + k] = pos, A.ones[s0 + k] = (k & 1) ? acc : acc + pos;
      ++k;
    }
    if (tid == 0) {                                                              // the last boundary is h w
      const int total = L.part[PG_THREADS], sum = L.part2[PG_THREADS];
      if (total < cap) {
        A.bounds[s0 + total] = (int)hw;
        A.ones[s0 + total] = (total & 1) ? sum + (int)hw : sum;
        A.count[o] = total + 1, A.status[o] = PG_ST_OK;
      } else {
        A.count[o] = 0, A.status[o] = PG_ST_SLOTS;
      }
    }
  });
}

}  // namespace univs
#endif  // UNIVS_POLYGON_CORE_H
