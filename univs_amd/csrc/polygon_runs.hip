// Polygon segmentations to run-length boundaries (include/univs_polygons_hip.h), gfx950: one workgroup of 256 lanes per object, all
// objects of an annotation file in one launch.  Neither a dense plane nor a per-point array exists in global memory: a lane recomputes
// the point it needs from the scaled vertices in LDS, and only the crossings -- a fifth of the columns a polygon's outline passes -- are
// kept, in LDS, until they leave as boundaries.
//
// The text of the work, its schedule and every bounds decision are csrc/polygon_core.h, which tools/polygon_host.cpp compiles for the
// host with a serial copy of the executor below.  Compiled without contraction to fma (the pragma at the head of polygon_core.h).
//
// LDS: flags 2 KB | X, Y, off 48 KB | keys 64 KB | two scan rows 2 KB | counters | coverage 32 KB: 151 600 bytes, one workgroup per CU.
#include "launchers.h"
#include "polygon_core.h"

namespace univs {

struct PgGroup {
  template <class F>
  __device__ __forceinline__ void each(F f) {
    f((int)threadIdx.x);
    __syncthreads();
  }
  __device__ __forceinline__ int read(const int* p) {
    const int v = *p;
    __syncthreads();
    return v;
  }
  __device__ __forceinline__ int append(int* p) { return atomicAdd(p, 1); }
};

constexpr size_t PG_LDS_BYTES = sizeof(unsigned long long) * PG_THREADS + sizeof(int) * PG_LDS_INTS + sizeof(unsigned) * PG_MAX_KEYS +
                                sizeof(int) * 2 * (PG_THREADS + 1) + sizeof(int) * 4 + sizeof(unsigned short) * PG_MAX_KEYS;

__global__ __launch_bounds__(PG_THREADS) void polygons_to_runs_kernel(PgArgs A) {
  extern __shared__ unsigned long long pg_lds[];
  PgLds L;
  L.flags = pg_lds;
  L.X = reinterpret_cast<int*>(L.flags + PG_THREADS);
  L.Y = L.X + (PG_MAX_VERTS + 1);
  L.off = L.Y + (PG_MAX_VERTS + 1);
  L.keys = reinterpret_cast<unsigned*>(L.off + (PG_MAX_VERTS + 1));
  L.part = reinterpret_cast<int*>(L.keys + PG_MAX_KEYS);
  L.part2 = L.part + (PG_THREADS + 1);
  L.ctr = L.part2 + (PG_THREADS + 1);
  L.cover = reinterpret_cast<unsigned short*>(L.ctr + 4);
  PgGroup ex;
  pg_object(ex, A, (int)blockIdx.x, L);
}

int polygons_to_runs(const double* xy, const int* poly_start, const int* obj_start, const int* size, const long long* slot, long long n_points,
                     int P, int N, long long cap_total, int* bounds, int* ones, int* count, int* status, hipStream_t st) {
  // above the default limit of dynamic LDS the kernel is allowed its image, once per device (as csrc/text_attn.hip does)
  static bool asked[64] = {};
  static hipError_t answer[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const int s = dev & 63;
  if (!asked[s]) {
    answer[s] = hipFuncSetAttribute(reinterpret_cast<const void*>(&polygons_to_runs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)PG_LDS_BYTES);
    asked[s] = answer[s] == hipSuccess;
  }
  if (answer[s] != hipSuccess) {
    set_error("polygons_to_runs: %zu bytes of LDS refused: %s", PG_LDS_BYTES, hipGetErrorString(answer[s]));
    return UNIVS_ERR_LAUNCH;
  }
  PgArgs A;
  A.xy = xy, A.poly_start = poly_start, A.obj_start = obj_start, A.size = size, A.slot = slot;
  A.bounds = bounds, A.ones = ones, A.count = count, A.status = status;
  A.n_points = n_points, A.cap_total = cap_total, A.P = P, A.N = N;
  hipLaunchKernelGGL(polygons_to_runs_kernel, dim3((unsigned)N), dim3(PG_THREADS), PG_LDS_BYTES, st, A);
  return check_launch("polygons_to_runs");
}

}  // namespace univs
