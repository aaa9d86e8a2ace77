// Cascaded occupancy grids and cone-stepped packed marching of the hash field.  Contract: include/lab4d_conemarch.h; every rule and all of the
// arithmetic: conemarch_math.hpp (over occgrid_math.hpp and ray_math.hpp), shared with the CPU twin
// tests/host_harness/conemarch/conemarch_host.cpp, to which these kernels are held word for word.  Nothing here reads back or allocates: every
// entry point can be captured in a hipGraph.
#include "common.hpp"
#include "conemarch_math.hpp"

namespace lab4d {
namespace occ = lab4d_occ;
namespace cone = lab4d_cone;

// One lane per point.  The boxes are read through the scalar cache (the address is the same in every lane), the edges are formed once per lane.
__global__ void __launch_bounds__(256) k_occgrid_cascade_mask(const float* __restrict__ xyz, const float* __restrict__ delta, const float* __restrict__ aabbs,
                                                               const uint32_t* __restrict__ bits, int K, int G, long S, uint8_t* __restrict__ mask,
                                                               int32_t* __restrict__ level) {
  const cone::Edges E = cone::cascade_edges(aabbs, K, G);
  for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (long)gridDim.x * blockDim.x) {
    const float p[3] = {xyz[3 * s], xyz[3 * s + 1], xyz[3 * s + 2]};
    int lv;
    const bool keep = cone::cascade_keep(p, delta ? delta[s] : 0.f, aabbs, bits, E, K, G, &lv);
    mask[s] = keep ? 1 : 0;
    if (level) level[s] = lv;
  }
}

// One lane per ray, as k_packed_march_count: the clip against the outermost box, then the ray's own recurrence of steps.
__global__ void __launch_bounds__(256) k_packed_march_cone_count(const float* __restrict__ origin, const float* __restrict__ dir,
                                                                  const float* __restrict__ t_range, const float* __restrict__ aabbs,
                                                                  const uint32_t* __restrict__ bits, int K, int G, long R, float cone_angle, float dt_min,
                                                                  float dt_max, int k_max, int32_t* __restrict__ ray_count) {
  const cone::Edges E = cone::cascade_edges(aabbs, K, G);
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    const float o[3] = {origin[3 * r], origin[3 * r + 1], origin[3 * r + 2]};
    const float d[3] = {dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    ray_count[r] = cone::march_cone_ray(o, d, t_range[2 * r], t_range[2 * r + 1], aabbs, bits, E, K, G, cone_angle, dt_min, dt_max, k_max,
                                        [](int, float, float, float, const float*, int) {});
  }
}

// The same march again; row i of ray r goes to ray_start[r] + i when that row lies below the capacity.  The last ray knows the total.
__global__ void __launch_bounds__(256) k_packed_march_cone_write(const float* __restrict__ origin, const float* __restrict__ dir,
                                                                  const float* __restrict__ t_range, const float* __restrict__ aabbs,
                                                                  const uint32_t* __restrict__ bits, int K, int G, long R, float cone_angle, float dt_min,
                                                                  float dt_max, int k_max, const int32_t* __restrict__ ray_start, long cap,
                                                                  float* __restrict__ t_out, float* __restrict__ steps, float* __restrict__ deltas,
                                                                  float* __restrict__ xyz, float* __restrict__ dirs, int32_t* __restrict__ ray_idx,
                                                                  int32_t* __restrict__ level, int32_t* __restrict__ ray_count_out,
                                                                  int32_t* __restrict__ total, uint8_t* __restrict__ overflow) {
  const cone::Edges E = cone::cascade_edges(aabbs, K, G);
  if (R == 0 && blockIdx.x == 0 && threadIdx.x == 0) { *total = 0; *overflow = 0; }
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    const float o[3] = {origin[3 * r], origin[3 * r + 1], origin[3 * r + 2]};
    const float d[3] = {dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    const float len = cone::dir_length(d);
    const float u[3] = {len > 0.f ? occ::div_rn(d[0], len) : 0.f, len > 0.f ? occ::div_rn(d[1], len) : 0.f, len > 0.f ? occ::div_rn(d[2], len) : 0.f};
    const long start = ray_start[r];
    const int n = cone::march_cone_ray(o, d, t_range[2 * r], t_range[2 * r + 1], aabbs, bits, E, K, G, cone_angle, dt_min, dt_max, k_max,
                                       [&](int i, float t, float s, float delta, const float* p, int lv) {
      const long row = start + i;
      if (row < 0 || row >= cap) return;
      t_out[row] = t;
      steps[row] = s;
      deltas[row] = delta;
      xyz[3 * row] = p[0]; xyz[3 * row + 1] = p[1]; xyz[3 * row + 2] = p[2];
      dirs[3 * row] = u[0]; dirs[3 * row + 1] = u[1]; dirs[3 * row + 2] = u[2];
      ray_idx[row] = (int32_t)r;
      level[row] = lv;
    });
    ray_count_out[r] = cone::clamp_count((int)start, n, (int)cap);
    if (r == R - 1) {
      const long tot = start + n;
      *total = (int32_t)tot;
      *overflow = tot > cap ? 1 : 0;
    }
  }
}

// rows in [min(total, cap), cap): parked outside box K - 1 (runs behind k_packed_march_cone_write on the same stream)
__global__ void __launch_bounds__(256) k_packed_cone_park(const float* __restrict__ aabbs, int K, const int32_t* __restrict__ total, long cap,
                                                           float* __restrict__ t_out, float* __restrict__ steps, float* __restrict__ deltas,
                                                           float* __restrict__ xyz, float* __restrict__ dirs, int32_t* __restrict__ ray_idx,
                                                           int32_t* __restrict__ level) {
  const float* aabb = aabbs + 6 * (K - 1);
  const float box[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
  float p[3];
  cone::park_point(box, p);
  long first = *total;
  if (first < 0) first = 0;
  for (long row = first + (long)blockIdx.x * blockDim.x + threadIdx.x; row < cap; row += (long)gridDim.x * blockDim.x) {
    t_out[row] = 0.f;
    steps[row] = 0.f;
    deltas[row] = 0.f;
    xyz[3 * row] = p[0]; xyz[3 * row + 1] = p[1]; xyz[3 * row + 2] = p[2];
    dirs[3 * row] = 0.f; dirs[3 * row + 1] = 0.f; dirs[3 * row + 2] = 1.f;
    ray_idx[row] = -1;
    level[row] = -1;
  }
}

}  // namespace lab4d
using namespace lab4d;

static int check_cascade(const char* what, int K, int G) {
  LAB4D_REQUIRE(K >= lab4d_cone::kMinK && K <= lab4d_cone::kMaxK, "%s: K = %d outside [%d, %d]", what, K, lab4d_cone::kMinK, lab4d_cone::kMaxK);
  LAB4D_REQUIRE(G >= lab4d_occ::kMinG && G <= lab4d_occ::kMaxG, "%s: G = %d outside [%d, %d]", what, G, lab4d_occ::kMinG, lab4d_occ::kMaxG);
  LAB4D_REQUIRE(K == 1 || G % 2 == 0, "%s: G = %d must be even with K = %d > 1 levels", what, G, K);
  return LAB4D_OK;
}

static int check_cone_march(const char* what, int K, int G, long R, float cone_angle, float dt_min, float dt_max, int k_max) {
  LAB4D_REQUIRE(R >= 0, "%s: R < 0", what);
  if (int e = check_cascade(what, K, G)) return e;
  LAB4D_REQUIRE(cone_angle >= 0.f && lab4d_occ::finite_f(cone_angle), "%s: cone = %g must be finite and >= 0", what, (double)cone_angle);
  LAB4D_REQUIRE(dt_min > 0.f && lab4d_occ::finite_f(dt_min), "%s: dt_min = %g must be finite and > 0", what, (double)dt_min);
  LAB4D_REQUIRE(dt_max >= dt_min && lab4d_occ::finite_f(dt_max), "%s: dt_max = %g must be finite and >= dt_min = %g", what, (double)dt_max, (double)dt_min);
  LAB4D_REQUIRE(k_max >= 1, "%s: k_max = %d must be >= 1", what, k_max);
  LAB4D_REQUIRE(R * (long)k_max < (1L << 31), "%s: R * k_max = %ld * %d does not fit 31 bits", what, R, k_max);
  return LAB4D_OK;
}

extern "C" int lab4d_occgrid_cascade_mask(const float* xyz, const float* delta, const float* aabbs, const uint32_t* bits, int K, int G, long S,
                                          uint8_t* mask, int32_t* level, void* stream) {
  LAB4D_REQUIRE(S >= 0, "occgrid_cascade_mask: S < 0");
  if (int e = check_cascade("occgrid_cascade_mask", K, G)) return e;
  if (S == 0) return LAB4D_OK;
  LAB4D_REQUIRE(xyz && aabbs && bits && mask, "occgrid_cascade_mask: null pointer");
  hipLaunchKernelGGL(k_occgrid_cascade_mask, dim3(grid_1d(S, 256, 8192)), dim3(256), 0, (hipStream_t)stream, xyz, delta, aabbs, bits, K, G, S, mask, level);
  return check_launch("occgrid_cascade_mask");
}

extern "C" int lab4d_packed_march_cone_count(const float* origin, const float* dir, const float* t_range, const float* aabbs, const uint32_t* bits,
                                             int K, int G, long R, float cone_angle, float dt_min, float dt_max, int k_max, int32_t* ray_count,
                                             void* stream) {
  if (int e = check_cone_march("packed_march_cone_count", K, G, R, cone_angle, dt_min, dt_max, k_max)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(origin && dir && t_range && aabbs && bits && ray_count, "packed_march_cone_count: null pointer");
  hipLaunchKernelGGL(k_packed_march_cone_count, dim3(grid_1d(R, 256, 16384)), dim3(256), 0, (hipStream_t)stream, origin, dir, t_range, aabbs, bits, K, G, R,
                     cone_angle, dt_min, dt_max, k_max, ray_count);
  return check_launch("packed_march_cone_count");
}

extern "C" int lab4d_packed_march_cone_write(const float* origin, const float* dir, const float* t_range, const float* aabbs, const uint32_t* bits,
                                             int K, int G, long R, float cone_angle, float dt_min, float dt_max, int k_max, const int32_t* ray_start,
                                             long cap, float* t, float* steps, float* deltas, float* xyz, float* dirs, int32_t* ray_idx,
                                             int32_t* level, int32_t* ray_count_out, int32_t* total, uint8_t* overflow, void* stream) {
  if (int e = check_cone_march("packed_march_cone_write", K, G, R, cone_angle, dt_min, dt_max, k_max)) return e;
  LAB4D_REQUIRE(cap >= 0 && cap < (1L << 31), "packed_march_cone_write: cap = %ld outside [0, 2^31)", cap);
  LAB4D_REQUIRE(aabbs && total && overflow, "packed_march_cone_write: null pointer");
  LAB4D_REQUIRE(R == 0 || (origin && dir && t_range && bits && ray_start && ray_count_out), "packed_march_cone_write: null pointer");
  LAB4D_REQUIRE(cap == 0 || (t && steps && deltas && xyz && dirs && ray_idx && level), "packed_march_cone_write: null packed buffer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_packed_march_cone_write, dim3(grid_1d(R, 256, 16384)), dim3(256), 0, st, origin, dir, t_range, aabbs, bits, K, G, R, cone_angle, dt_min,
                     dt_max, k_max, ray_start, cap, t, steps, deltas, xyz, dirs, ray_idx, level, ray_count_out, total, overflow);
  if (int e = check_launch("packed_march_cone_write")) return e;
  if (cap == 0) return LAB4D_OK;
  hipLaunchKernelGGL(k_packed_cone_park, dim3(grid_1d(cap, 256, 16384)), dim3(256), 0, st, aabbs, K, total, cap, t, steps, deltas, xyz, dirs, ray_idx, level);
  return check_launch("packed_march_cone_write (park)");
}
