// Merge of two packed sample lists per ray by depth, and the gather of per-row values through it.  Contract: include/lab4d_pmerge.h; every
// rule: pmerge_math.hpp (over prune_math.hpp / packed_math.hpp), shared with the CPU twin tests/host_harness/pmerge/pmerge_host.cpp, to which
// the kernels are held word for word.  The write pass has the partition of k_packed_composite_fwd: one 64-lane wave per ray, four rays per
// 256-thread block, grid-stride; the lanes stride over the ray's A rows and then over its B rows, and every row finds its place with one
// binary search over the ray's rows of the other list (at most k_max = 1024 of them by default: ten steps, on lines the wave shares).  No
// shuffles, no ballots, no LDS, no atomics; nothing reads back or allocates: every entry point can be captured in a hipGraph.
#include "common.hpp"
#include "pmerge_math.hpp"

namespace lab4d {
namespace pk = lab4d_packed;
namespace pm = lab4d_pmerge;

__global__ void __launch_bounds__(256) k_packed_merge_count(const int32_t* __restrict__ start_a, const int32_t* __restrict__ count_a, long Pa,
                                                             const int32_t* __restrict__ start_b, const int32_t* __restrict__ count_b, long Pb, long R,
                                                             int32_t* __restrict__ ray_count) {
  for (long ray = (long)blockIdx.x * blockDim.x + threadIdx.x; ray < R; ray += (long)gridDim.x * blockDim.x)
    ray_count[ray] = pm::rows_of(start_a, count_a, ray, Pa).n + pm::rows_of(start_b, count_b, ray, Pb).n;
}

// pos_a, pos_b = -1 (runs in front of k_packed_merge_write on the same stream: the rows that no ray owns, and those behind the capacity, keep it)
__global__ void __launch_bounds__(256) k_packed_merge_clear(long Pa, long Pb, int32_t* __restrict__ pos_a, int32_t* __restrict__ pos_b) {
  for (long row = (long)blockIdx.x * blockDim.x + threadIdx.x; row < Pa + Pb; row += (long)gridDim.x * blockDim.x) {
    if (row < Pa) pos_a[row] = -1;
    else pos_b[row - Pa] = -1;
  }
}

// The rows of one list of one ray: row i of `mine` goes to merged row base + place, when that row lies below the capacity.
template <bool kFromB>
__device__ __forceinline__ void merge_rows_of(const float* __restrict__ t_mine, const float* __restrict__ deltas_mine, pm::Rows mine,
                                              const float* __restrict__ t_other, pm::Rows other, long Pa, long ray, long base, long cap, int lane,
                                              float* __restrict__ t, float* __restrict__ deltas, int32_t* __restrict__ ray_idx, int32_t* __restrict__ src,
                                              int32_t* __restrict__ pos_mine) {
  for (int i = lane; i < mine.n; i += 64) {
    const long row = mine.s + i;
    const float x = t_mine[row];
    const long dst = base + (kFromB ? pm::place_b(i, x, t_other + other.s, other.n) : pm::place_a(i, x, t_other + other.s, other.n));
    if (dst >= 0 && dst < cap) {
      t[dst] = x;
      deltas[dst] = deltas_mine[row];
      ray_idx[dst] = (int32_t)ray;
      src[dst] = pm::src_of(kFromB, row, Pa);
      pos_mine[row] = (int32_t)dst;
    }
  }
}

// The last ray knows the total.
__global__ void __launch_bounds__(256) k_packed_merge_write(const float* __restrict__ t_a, const float* __restrict__ deltas_a, const int32_t* __restrict__ start_a,
                                                             const int32_t* __restrict__ count_a, long Pa, const float* __restrict__ t_b,
                                                             const float* __restrict__ deltas_b, const int32_t* __restrict__ start_b,
                                                             const int32_t* __restrict__ count_b, long Pb, long R, const int32_t* __restrict__ ray_start, long cap,
                                                             float* __restrict__ t, float* __restrict__ deltas, int32_t* __restrict__ ray_idx,
                                                             int32_t* __restrict__ src, int32_t* __restrict__ pos_a, int32_t* __restrict__ pos_b,
                                                             int32_t* __restrict__ ray_count_out, int32_t* __restrict__ total, uint8_t* __restrict__ overflow) {
  const int lane = threadIdx.x & 63;
  if (R == 0 && blockIdx.x == 0 && threadIdx.x == 0) { *total = 0; *overflow = 0; }
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const pm::Rows ra = pm::rows_of(start_a, count_a, ray, Pa), rb = pm::rows_of(start_b, count_b, ray, Pb);
    const long base = ray_start[ray];
    merge_rows_of<false>(t_a, deltas_a, ra, t_b, rb, Pa, ray, base, cap, lane, t, deltas, ray_idx, src, pos_a);
    merge_rows_of<true>(t_b, deltas_b, rb, t_a, ra, Pa, ray, base, cap, lane, t, deltas, ray_idx, src, pos_b);
    if (lane == 0) {
      const int n = ra.n + rb.n;
      ray_count_out[ray] = pk::clamp_count((int)base, n, (int)cap);
      if (ray == R - 1) {
        const long tot = base + n;
        *total = (int32_t)tot;
        *overflow = tot > cap ? 1 : 0;
      }
    }
  }
}

// rows in [min(total, cap), cap): parked (runs behind k_packed_merge_write on the same stream)
__global__ void __launch_bounds__(256) k_packed_merge_park(const int32_t* __restrict__ total, long cap, float* __restrict__ t, float* __restrict__ deltas,
                                                            int32_t* __restrict__ ray_idx, int32_t* __restrict__ src) {
  long first = *total;
  if (first < 0) first = 0;
  for (long row = first + (long)blockIdx.x * blockDim.x + threadIdx.x; row < cap; row += (long)gridDim.x * blockDim.x) {
    t[row] = 0.f;
    deltas[row] = 0.f;
    ray_idx[row] = -1;
    src[row] = -1;
  }
}

// lanes over the n * C values of out: consecutive lanes read consecutive channels of a source row and write consecutive words
__global__ void __launch_bounds__(256) k_packed_merge_gather(const float* __restrict__ a, long Pa, const float* __restrict__ b, long Pb,
                                                              const int32_t* __restrict__ idx, long n, int C, float* __restrict__ out) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n * C; e += (long)gridDim.x * blockDim.x) {
    const long j = e / C;
    out[e] = pm::gather_value(a, Pa, b, Pb, idx[j], C, (int)(e - j * C));
  }
}

}  // namespace lab4d
using namespace lab4d;

static int check_lists(const char* what, long R, long Pa, long Pb) {
  LAB4D_REQUIRE(R >= 0 && R < (1L << 31), "%s: R = %ld outside [0, 2^31)", what, R);
  LAB4D_REQUIRE(Pa >= 0 && Pb >= 0 && Pa + Pb < (1L << 31), "%s: Pa = %ld, Pb = %ld: both must be >= 0 and Pa + Pb < 2^31", what, Pa, Pb);
  return LAB4D_OK;
}

extern "C" int lab4d_packed_merge_count(const int32_t* start_a, const int32_t* count_a, long Pa, const int32_t* start_b, const int32_t* count_b, long Pb,
                                        long R, int32_t* ray_count, void* stream) {
  if (int e = check_lists("packed_merge_count", R, Pa, Pb)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(start_a && count_a && start_b && count_b && ray_count, "packed_merge_count: null start / count / ray_count");
  hipLaunchKernelGGL(k_packed_merge_count, dim3(grid_1d(R, 256, 16384)), dim3(256), 0, (hipStream_t)stream, start_a, count_a, Pa, start_b, count_b, Pb, R,
                     ray_count);
  return check_launch("packed_merge_count");
}

extern "C" int lab4d_packed_merge_write(const float* t_a, const float* deltas_a, const int32_t* start_a, const int32_t* count_a, long Pa, const float* t_b,
                                        const float* deltas_b, const int32_t* start_b, const int32_t* count_b, long Pb, long R, const int32_t* ray_start,
                                        long cap, float* t, float* deltas, int32_t* ray_idx, int32_t* src, int32_t* pos_a, int32_t* pos_b,
                                        int32_t* ray_count_out, int32_t* total, uint8_t* overflow, void* stream) {
  if (int e = check_lists("packed_merge_write", R, Pa, Pb)) return e;
  LAB4D_REQUIRE(cap >= 0 && cap < (1L << 31), "packed_merge_write: cap = %ld outside [0, 2^31)", cap);
  LAB4D_REQUIRE(total && overflow, "packed_merge_write: null total / overflow");
  LAB4D_REQUIRE(R == 0 || (start_a && count_a && start_b && count_b && ray_start && ray_count_out), "packed_merge_write: null start / count / ray_start");
  LAB4D_REQUIRE(Pa == 0 || (t_a && deltas_a && pos_a), "packed_merge_write: null t_a / deltas_a / pos_a");
  LAB4D_REQUIRE(Pb == 0 || (t_b && deltas_b && pos_b), "packed_merge_write: null t_b / deltas_b / pos_b");
  LAB4D_REQUIRE(cap == 0 || (t && deltas && ray_idx && src), "packed_merge_write: null merged buffer");
  hipStream_t st = (hipStream_t)stream;
  if (Pa + Pb > 0) {
    hipLaunchKernelGGL(k_packed_merge_clear, dim3(grid_1d(Pa + Pb, 256, 16384)), dim3(256), 0, st, Pa, Pb, pos_a, pos_b);
    if (int e = check_launch("packed_merge_write (clear)")) return e;
  }
  hipLaunchKernelGGL(k_packed_merge_write, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, st, t_a, deltas_a, start_a, count_a, Pa, t_b, deltas_b, start_b, count_b, Pb, R,
                     ray_start, cap, t, deltas, ray_idx, src, pos_a, pos_b, ray_count_out, total, overflow);
  if (int e = check_launch("packed_merge_write")) return e;
  if (cap == 0) return LAB4D_OK;
  hipLaunchKernelGGL(k_packed_merge_park, dim3(grid_1d(cap, 256, 16384)), dim3(256), 0, st, total, cap, t, deltas, ray_idx, src);
  return check_launch("packed_merge_write (park)");
}

extern "C" int lab4d_packed_merge_gather(const float* a, long Pa, const float* b, long Pb, const int32_t* idx, long n, int C, float* out, void* stream) {
  LAB4D_REQUIRE(Pa >= 0 && Pb >= 0 && Pa + Pb < (1L << 31), "packed_merge_gather: Pa = %ld, Pb = %ld: both must be >= 0 and Pa + Pb < 2^31", Pa, Pb);
  LAB4D_REQUIRE(n >= 0 && n < (1L << 31), "packed_merge_gather: n = %ld outside [0, 2^31)", n);
  LAB4D_REQUIRE(C >= 1 && C <= 64, "packed_merge_gather: C = %d outside [1, 64]", C);
  if (n == 0) return LAB4D_OK;
  LAB4D_REQUIRE(idx && out, "packed_merge_gather: null idx / out");
  hipLaunchKernelGGL(k_packed_merge_gather, dim3(grid_1d(n * C, 256, 16384)), dim3(256), 0, (hipStream_t)stream, a, Pa, b, Pb, idx, n, C, out);
  return check_launch("packed_merge_gather");
}
