// The polygon rasteriser of the device, run on the host: this program compiles univs_amd/csrc/polygon_core.h, the very header
// csrc/polygon_runs.hip compiles, and runs every object by the kernel's lane schedule -- each phase for lane 0 .. 255 in turn, a barrier
// being the end of the loop.  It is the CPU evidence that the bounds decisions hold before an untrusted table or coordinate reaches a
// GPU: built with -fsanitize=address,undefined, the tables, the coordinates, the output slots and every LDS array live in heap blocks of
// exactly their sizes, so a load or store outside one is a sanitizer report (tests/test_polygon_host_cpu.py).
//
//   polygon_host < call
// call (little endian): int64 N, P, n_points, cap_total; int32 obj_start[N + 1], poly_start[P + 1], size[2 N]; int64 slot[N + 1];
// float64 xy[2 n_points].  One line per object: "<status> <count> : <boundaries> : <ones>".
//   c++ -O1 -g -std=c++17 -ffp-contract=off [-fsanitize=address,undefined] tools/polygon_host.cpp -o polygon_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../univs_amd/csrc/polygon_core.h"

struct Serial {
  template <class F>
  void each(F f) {
    for (int tid = 0; tid < univs::PG_THREADS; ++tid) f(tid);
  }
  int read(const int* p) { return *p; }
  int append(int* p) { return (*p)++; }
};

template <class T>
static T* block(size_t n) {
  T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));   // exact: the sanitizer sees the first element outside
  if (!p) {
    std::fprintf(stderr, "polygon_host: out of memory\n");
    std::exit(2);
  }
  std::memset(p, 0, n * sizeof(T));
  return p;
}

template <class T>
static T* read_block(size_t n) {
  T* p = block<T>(n);
  if (n && std::fread(p, sizeof(T), n, stdin) != n) {
    std::fprintf(stderr, "polygon_host: short input\n");
    std::exit(2);
  }
  return p;
}

int main() {
  long long head[4];
  if (std::fread(head, sizeof(long long), 4, stdin) != 4 || head[0] < 0 || head[1] < 0 || head[2] < 0 || head[3] < 0 ||
      head[0] >= (1LL << 28) || head[1] >= (1LL << 28) || head[2] >= (1LL << 28) || head[3] >= (1LL << 28)) {
    std::fprintf(stderr, "polygon_host: bad header\n");
    return 2;
  }
  using namespace univs;
  PgArgs A;
  A.N = (int)head[0], A.P = (int)head[1], A.n_points = head[2], A.cap_total = head[3];
  A.obj_start = read_block<int>((size_t)A.N + 1);
  A.poly_start = read_block<int>((size_t)A.P + 1);
  A.size = read_block<int>(2 * (size_t)A.N);
  A.slot = read_block<long long>((size_t)A.N + 1);
  A.xy = read_block<double>(2 * (size_t)A.n_points);
  A.bounds = block<int>((size_t)A.cap_total);
  A.ones = block<int>((size_t)A.cap_total);
  A.count = block<int>((size_t)A.N);
  A.status = block<int>((size_t)A.N);
  PgLds L;
  L.X = block<int>(PG_MAX_VERTS + 1), L.Y = block<int>(PG_MAX_VERTS + 1), L.off = block<int>(PG_MAX_VERTS + 1);
  L.cover = block<unsigned short>(PG_MAX_KEYS);
  L.keys = block<unsigned>(PG_MAX_KEYS);
  L.part = block<int>(PG_THREADS + 1);
  L.part2 = block<int>(PG_THREADS + 1);
  L.flags = block<unsigned long long>(PG_THREADS);
  L.ctr = block<int>(4);
  Serial ex;
  for (int o = 0; o < A.N; ++o) {
    pg_object<Serial>(ex, A, o, L);
    std::printf("%d %d :", A.status[o], A.count[o]);
    const long long s0 = pg_clampl(A.slot[o], 0, A.cap_total);
    for (int k = 0; k < A.count[o]; ++k) std::printf(" %d", A.bounds[s0 + k]);
    std::printf(" :");
    for (int k = 0; k < A.count[o]; ++k) std::printf(" %d", A.ones[s0 + k]);
    std::printf("\n");
  }
  for (const void* p : {(const void*)A.obj_start, (const void*)A.poly_start, (const void*)A.size, (const void*)A.slot, (const void*)A.xy,
                        (const void*)A.bounds, (const void*)A.ones, (const void*)A.count, (const void*)A.status, (const void*)L.X,
                        (const void*)L.Y, (const void*)L.off, (const void*)L.cover, (const void*)L.keys, (const void*)L.part,
                        (const void*)L.part2, (const void*)L.flags, (const void*)L.ctr})
    std::free(const_cast<void*>(p));
  return 0;
}
