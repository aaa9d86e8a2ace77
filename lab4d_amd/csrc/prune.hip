// Pruning of a packed sample list by transmittance and opacity.  Contract: include/lab4d_prune.h; every rule: prune_math.hpp (over
// packed_math.hpp), shared with the CPU twin tests/host_harness/prune/prune_host.cpp, to which both kernels are held word for word.  The partition
// is k_packed_composite_fwd's: one 64-lane wave per ray, four rays per 256-thread block, grid-stride, lanes over the ray's consecutive rows
// 64 at a time.  Every loop bound is the wave's own ray, so the shuffles and ballots run with all 64 lanes.  No LDS, no atomics; nothing
// reads back or allocates: both entry points can be captured in a hipGraph.
#include "common.hpp"
#include "prune_math.hpp"

namespace lab4d {
namespace pk = lab4d_packed;
namespace pr = lab4d_prune;

__global__ void __launch_bounds__(256) k_packed_prune_count(const float* __restrict__ density, const float* __restrict__ deltas,
                                                             const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count, long R, long P,
                                                             float tau_stop, float tau_min, uint8_t* __restrict__ keep, int32_t* __restrict__ new_count) {
  const int lane = threadIdx.x & 63;
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const pr::Rows rr = pr::rows_of(ray_start, ray_count, ray, P);
    float carry = 0.f;
    int kept = 0, j0 = 0;
    bool stopped = false;
    for (; j0 < rr.n && !stopped; j0 += 64) {
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      const float tau = live ? pr::tau_of(density[row], deltas[row]) : 0.f;
      const float incl = wave_scan_incl(tau, lane) + carry;
      float excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = carry;
      carry = __shfl(incl, 63, 64);
      const unsigned long long stop = __ballot(pr::stops(live, excl, tau_stop));
      const bool k = pr::keeps(live, lane, pr::first_lane(stop), tau, tau_min);
      if (live) keep[row] = k ? 1 : 0;
      kept += __popcll(__ballot(k));  // (the same value in every lane)
      stopped = stop != 0ull;
    }
    for (; j0 < rr.n; j0 += 64)  // behind the chunk that holds the stop: nothing is read any more
      if (j0 + lane < rr.n) keep[rr.s + j0 + lane] = 0;
    if (lane == 0) new_count[ray] = kept;
  }
}

// Survivor number n + rank of the ray goes to row new_start[ray] + n + rank when that row lies below the capacity.  The last ray knows the total.
__global__ void __launch_bounds__(256) k_packed_prune_write(const uint8_t* __restrict__ keep, const int32_t* __restrict__ ray_start,
                                                             const int32_t* __restrict__ ray_count, const int32_t* __restrict__ new_start, long R, long P,
                                                             long cap, const float* __restrict__ t, const float* __restrict__ deltas,
                                                             const float* __restrict__ xyz, const float* __restrict__ dirs, float* __restrict__ t_out,
                                                             float* __restrict__ deltas_out, float* __restrict__ xyz_out, float* __restrict__ dirs_out,
                                                             int32_t* __restrict__ ray_idx_out, int32_t* __restrict__ src_row_out,
                                                             int32_t* __restrict__ new_count_out, int32_t* __restrict__ total, uint8_t* __restrict__ overflow) {
  const int lane = threadIdx.x & 63;
  if (R == 0 && blockIdx.x == 0 && threadIdx.x == 0) { *total = 0; *overflow = 0; }
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const pr::Rows rr = pr::rows_of(ray_start, ray_count, ray, P);
    const long base = new_start[ray];
    int n = 0;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      const bool k = live && keep[row] != 0;
      const unsigned long long bal = __ballot(k);
      const long dst = base + n + pr::rank_of(bal, lane);
      if (k && dst >= 0 && dst < cap) {
        t_out[dst] = t[row];
        deltas_out[dst] = deltas[row];
        xyz_out[3 * dst] = xyz[3 * row]; xyz_out[3 * dst + 1] = xyz[3 * row + 1]; xyz_out[3 * dst + 2] = xyz[3 * row + 2];
        dirs_out[3 * dst] = dirs[3 * row]; dirs_out[3 * dst + 1] = dirs[3 * row + 1]; dirs_out[3 * dst + 2] = dirs[3 * row + 2];
        ray_idx_out[dst] = (int32_t)ray;
        src_row_out[dst] = (int32_t)row;
      }
      n += __popcll(bal);
    }
    if (lane == 0) {
      new_count_out[ray] = pk::clamp_count((int)base, n, (int)cap);
      if (ray == R - 1) {
        const long tot = base + n;
        *total = (int32_t)tot;
        *overflow = tot > cap ? 1 : 0;
      }
    }
  }
}

// rows in [min(total, cap), cap): parked as k_packed_park parks them, src_row = -1 (runs behind k_packed_prune_write on the same stream)
__global__ void __launch_bounds__(256) k_packed_prune_park(const float* __restrict__ aabb, const int32_t* __restrict__ total, long cap,
                                                            float* __restrict__ t_out, float* __restrict__ deltas_out, float* __restrict__ xyz_out,
                                                            float* __restrict__ dirs_out, int32_t* __restrict__ ray_idx_out, int32_t* __restrict__ src_row_out) {
  const float box[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
  float p[3];
  pk::park_point(box, p);
  long first = *total;
  if (first < 0) first = 0;
  for (long row = first + (long)blockIdx.x * blockDim.x + threadIdx.x; row < cap; row += (long)gridDim.x * blockDim.x) {
    t_out[row] = 0.f;
    deltas_out[row] = 0.f;
    xyz_out[3 * row] = p[0]; xyz_out[3 * row + 1] = p[1]; xyz_out[3 * row + 2] = p[2];
    dirs_out[3 * row] = 0.f; dirs_out[3 * row + 1] = 0.f; dirs_out[3 * row + 2] = 1.f;
    ray_idx_out[row] = -1;
    src_row_out[row] = -1;
  }
}

}  // namespace lab4d
using namespace lab4d;

static int check_rows(const char* what, long R, long P) {
  LAB4D_REQUIRE(R >= 0 && R < (1L << 31) && P >= 0 && P < (1L << 31), "%s: R = %ld or P = %ld outside [0, 2^31)", what, R, P);
  return LAB4D_OK;
}

extern "C" int lab4d_packed_prune_count(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P,
                                        float tau_stop, float tau_min, uint8_t* keep, int32_t* new_count, void* stream) {
  if (int e = check_rows("packed_prune_count", R, P)) return e;
  LAB4D_REQUIRE(tau_stop >= 0.f, "packed_prune_count: tau_stop = %g must be >= 0 or +inf", (double)tau_stop);  // (NaN compares false)
  LAB4D_REQUIRE(tau_min >= 0.f && lab4d_rn::finite_f(tau_min), "packed_prune_count: tau_min = %g must be finite and >= 0", (double)tau_min);
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start && ray_count && new_count, "packed_prune_count: null ray_start / ray_count / new_count");
  LAB4D_REQUIRE(P == 0 || (density && deltas && keep), "packed_prune_count: null density / deltas / keep");
  hipLaunchKernelGGL(k_packed_prune_count, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, density, deltas, ray_start, ray_count, R, P, tau_stop,
                     tau_min, keep, new_count);
  return check_launch("packed_prune_count");
}

extern "C" int lab4d_packed_prune_write(const uint8_t* keep, const int32_t* ray_start, const int32_t* ray_count, const int32_t* new_start, long R, long P,
                                        long cap, const float* aabb, const float* t, const float* deltas, const float* xyz, const float* dirs, float* t_out,
                                        float* deltas_out, float* xyz_out, float* dirs_out, int32_t* ray_idx_out, int32_t* src_row_out,
                                        int32_t* new_count_out, int32_t* total, uint8_t* overflow, void* stream) {
  if (int e = check_rows("packed_prune_write", R, P)) return e;
  LAB4D_REQUIRE(cap >= 0 && cap < (1L << 31), "packed_prune_write: cap = %ld outside [0, 2^31)", cap);
  LAB4D_REQUIRE(aabb && total && overflow, "packed_prune_write: null pointer");
  LAB4D_REQUIRE(R == 0 || (ray_start && ray_count && new_start && new_count_out), "packed_prune_write: null pointer");
  LAB4D_REQUIRE(R == 0 || P == 0 || (keep && t && deltas && xyz && dirs), "packed_prune_write: null source list");
  LAB4D_REQUIRE(cap == 0 || (t_out && deltas_out && xyz_out && dirs_out && ray_idx_out && src_row_out), "packed_prune_write: null packed buffer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_packed_prune_write, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, st, keep, ray_start, ray_count, new_start, R, P, cap, t, deltas, xyz, dirs,
                     t_out, deltas_out, xyz_out, dirs_out, ray_idx_out, src_row_out, new_count_out, total, overflow);
  if (int e = check_launch("packed_prune_write")) return e;
  if (cap == 0) return LAB4D_OK;
  hipLaunchKernelGGL(k_packed_prune_park, dim3(grid_1d(cap, 256, 16384)), dim3(256), 0, st, aabb, total, cap, t_out, deltas_out, xyz_out, dirs_out, ray_idx_out,
                     src_row_out);
  return check_launch("packed_prune_write (park)");
}
