// Importance resampling of a packed sample list per ray.  Contract: include/lab4d_presample.h; every rule: presample_math.hpp (over
// pmerge_math.hpp, prune_math.hpp and packed_math.hpp), shared with the CPU twin tests/host_harness/presample/presample_host.cpp, to which the
// two resample kernels are held word for word.  The partition is k_packed_composite_fwd's: one 64-lane wave per ray, four rays per
// 256-thread block, grid-stride.  The weights and the count kernel stride over the ray's consecutive rows 64 at a time with the carry of
// the sum scan; the write kernel strides over the ray's n_imp samples 64 at a time with the carry of the max scan, and every sample finds
// its source row with one binary search over the ray's prefixes (lines the wave shares).  Every loop bound is the wave's own ray, so the
// shuffles run with all 64 lanes.  No LDS, no atomics; nothing reads back or allocates: every entry point can be captured in a hipGraph.
#include "common.hpp"
#include "presample_math.hpp"

namespace lab4d {
namespace pk = lab4d_packed;
namespace ps = lab4d_presample;

__global__ void __launch_bounds__(256) k_packed_weights(const float* __restrict__ density, const float* __restrict__ deltas,
                                                         const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count, long R, long P,
                                                         float* __restrict__ w, float* __restrict__ trans) {
  const int lane = threadIdx.x & 63;
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const ps::Rows rr = ps::rows_of(ray_start, ray_count, ray, P);
    float carry = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      const float tau = live ? ps::tau_of(density[row], deltas[row]) : 0.f;
      const float incl = wave_scan_incl(tau, lane) + carry;
      float excl = __shfl_up(incl, 1, 64);
      if (lane == 0) excl = carry;
      carry = __shfl(incl, 63, 64);
      if (live) w[row] = pk::weight_of(tau, excl);
    }
    if (lane == 0 && trans) trans[ray] = pk::transmit_of(carry);
  }
}

__global__ void __launch_bounds__(256) k_packed_resample_count(const float* __restrict__ weights, const int32_t* __restrict__ ray_start,
                                                                const int32_t* __restrict__ ray_count, long R, long P, int n_imp, float eps,
                                                                float* __restrict__ cdf, float* __restrict__ mass, int32_t* __restrict__ new_count) {
  const int lane = threadIdx.x & 63;
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const ps::Rows rr = ps::rows_of(ray_start, ray_count, ray, P);
    float carry = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      const float m = live ? ps::mass_of(weights[row], eps) : 0.f;
      const float incl = wave_scan_incl(m, lane) + carry;
      carry = __shfl(incl, 63, 64);
      if (live) cdf[row] = incl;
    }
    if (lane == 0) {
      mass[ray] = carry;
      new_count[ray] = ps::count_of(rr.n, carry, n_imp);
    }
  }
}

// inclusive running maximum across the 64 lanes of a wave (later_of: the value of the lanes before is the first operand)
__device__ __forceinline__ float wave_scan_max(float v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float before = __shfl_up(v, o, 64);
    if (lane >= o) v = ps::later_of(before, v);
  }
  return v;
}

// Sample k of the ray goes to row new_start[ray] + k when that row lies below the capacity.  The last ray knows the total.
__global__ void __launch_bounds__(256) k_packed_resample_write(const float* __restrict__ weights, const float* __restrict__ cdf, const float* __restrict__ mass,
                                                                const float* __restrict__ t, const float* __restrict__ deltas,
                                                                const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count,
                                                                const int32_t* __restrict__ new_start, long R, long P, const float* __restrict__ origin,
                                                                const float* __restrict__ dir, const float* __restrict__ u, int n_imp, float eps, long cap,
                                                                float* __restrict__ t_out, float* __restrict__ deltas_out, float* __restrict__ xyz_out,
                                                                float* __restrict__ dirs_out, int32_t* __restrict__ ray_idx_out,
                                                                int32_t* __restrict__ src_row_out, int32_t* __restrict__ new_count_out,
                                                                int32_t* __restrict__ total, uint8_t* __restrict__ overflow) {
  const int lane = threadIdx.x & 63;
  if (R == 0 && blockIdx.x == 0 && threadIdx.x == 0) { *total = 0; *overflow = 0; }
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const ps::Rows rr = ps::rows_of(ray_start, ray_count, ray, P);
    const long base = new_start[ray];
    const float W = mass[ray];
    const int n = ps::count_of(rr.n, W, n_imp);
    if (n > 0) {
      const float o[3] = {origin[3 * ray], origin[3 * ray + 1], origin[3 * ray + 2]};
      const float d[3] = {dir[3 * ray], dir[3 * ray + 1], dir[3 * ray + 2]};
      const float len = pk::dir_length(d);
      const float unit[3] = {len > 0.f ? ps::div_rn(d[0], len) : 0.f, len > 0.f ? ps::div_rn(d[1], len) : 0.f, len > 0.f ? ps::div_rn(d[2], len) : 0.f};
      const float* C = cdf + rr.s;
      float carry = -lab4d_rn::inf_f();
      for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        const bool live = k < n;
        float tp = -lab4d_rn::inf_f(), span = 0.f;
        long row = 0;
        if (live) {
          const float q = ps::mul_rn(u ? ps::clamp01(u[ray * n_imp + k]) : ps::query_u(k, n_imp), W);
          const int i = ps::row_of(C, rr.n, q);
          row = rr.s + i;
          const float m = ps::mass_of(weights[row], eps), dl = deltas[row];
          tp = ps::t_of(t[row], ps::place_f(q, i > 0 ? C[i - 1] : 0.f, m), ps::width_of(dl, len));
          span = ps::span_of(dl, W, n_imp, m);
        }
        const float tk = ps::later_of(carry, wave_scan_max(tp, lane));
        carry = __shfl(tk, 63, 64);
        const long dst = base + k;
        if (live && dst >= 0 && dst < cap) {
          float p[3];
          pk::point_at(o, d, tk, p);
          t_out[dst] = tk;
          deltas_out[dst] = span;
          xyz_out[3 * dst] = p[0]; xyz_out[3 * dst + 1] = p[1]; xyz_out[3 * dst + 2] = p[2];
          dirs_out[3 * dst] = unit[0]; dirs_out[3 * dst + 1] = unit[1]; dirs_out[3 * dst + 2] = unit[2];
          ray_idx_out[dst] = (int32_t)ray;
          src_row_out[dst] = (int32_t)row;
        }
      }
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

// rows in [min(total, cap), cap): parked as k_packed_park parks them, src_row = -1 (runs behind k_packed_resample_write on the same stream)
__global__ void __launch_bounds__(256) k_packed_resample_park(const float* __restrict__ aabb, const int32_t* __restrict__ total, long cap,
                                                               float* __restrict__ t_out, float* __restrict__ deltas_out, float* __restrict__ xyz_out,
                                                               float* __restrict__ dirs_out, int32_t* __restrict__ ray_idx_out,
                                                               int32_t* __restrict__ src_row_out) {
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

static int check_resample(const char* what, long R, long P, int n_imp, float eps) {
  if (int e = check_rows(what, R, P)) return e;
  LAB4D_REQUIRE(n_imp >= 1, "%s: n_imp = %d must be >= 1", what, n_imp);
  LAB4D_REQUIRE(R * (long)n_imp < (1L << 31), "%s: R * n_imp = %ld * %d does not fit 31 bits", what, R, n_imp);
  LAB4D_REQUIRE(eps >= 0.f && lab4d_rn::finite_f(eps), "%s: eps = %g must be finite and >= 0", what, (double)eps);  // (NaN compares false)
  return LAB4D_OK;
}

extern "C" int lab4d_packed_weights(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P, float* w,
                                    float* trans, void* stream) {
  if (int e = check_rows("packed_weights", R, P)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start && ray_count, "packed_weights: null ray_start / ray_count");
  LAB4D_REQUIRE(P == 0 || (density && deltas && w), "packed_weights: null density / deltas / w");
  hipLaunchKernelGGL(k_packed_weights, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, density, deltas, ray_start, ray_count, R, P, w, trans);
  return check_launch("packed_weights");
}

extern "C" int lab4d_packed_resample_count(const float* weights, const int32_t* ray_start, const int32_t* ray_count, long R, long P, int n_imp, float eps,
                                           float* cdf, float* mass, int32_t* new_count, void* stream) {
  if (int e = check_resample("packed_resample_count", R, P, n_imp, eps)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start && ray_count && mass && new_count, "packed_resample_count: null ray_start / ray_count / mass / new_count");
  LAB4D_REQUIRE(P == 0 || (weights && cdf), "packed_resample_count: null weights / cdf");
  hipLaunchKernelGGL(k_packed_resample_count, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, weights, ray_start, ray_count, R, P, n_imp, eps, cdf,
                     mass, new_count);
  return check_launch("packed_resample_count");
}

extern "C" int lab4d_packed_resample_write(const float* weights, const float* cdf, const float* mass, const float* t, const float* deltas,
                                           const int32_t* ray_start, const int32_t* ray_count, const int32_t* new_start, long R, long P, const float* origin,
                                           const float* dir, const float* u, int n_imp, float eps, long cap, const float* aabb, float* t_out, float* deltas_out,
                                           float* xyz_out, float* dirs_out, int32_t* ray_idx_out, int32_t* src_row_out, int32_t* new_count_out, int32_t* total,
                                           uint8_t* overflow, void* stream) {
  if (int e = check_resample("packed_resample_write", R, P, n_imp, eps)) return e;
  LAB4D_REQUIRE(cap >= 0 && cap < (1L << 31), "packed_resample_write: cap = %ld outside [0, 2^31)", cap);
  LAB4D_REQUIRE(aabb && total && overflow, "packed_resample_write: null aabb / total / overflow");
  LAB4D_REQUIRE(R == 0 || (ray_start && ray_count && new_start && mass && origin && dir && new_count_out), "packed_resample_write: null per-ray pointer");
  LAB4D_REQUIRE(R == 0 || P == 0 || (weights && cdf && t && deltas), "packed_resample_write: null source list");
  LAB4D_REQUIRE(cap == 0 || (t_out && deltas_out && xyz_out && dirs_out && ray_idx_out && src_row_out), "packed_resample_write: null packed buffer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_packed_resample_write, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, st, weights, cdf, mass, t, deltas, ray_start, ray_count, new_start, R, P,
                     origin, dir, u, n_imp, eps, cap, t_out, deltas_out, xyz_out, dirs_out, ray_idx_out, src_row_out, new_count_out, total, overflow);
  if (int e = check_launch("packed_resample_write")) return e;
  if (cap == 0) return LAB4D_OK;
  hipLaunchKernelGGL(k_packed_resample_park, dim3(grid_1d(cap, 256, 16384)), dim3(256), 0, st, aabb, total, cap, t_out, deltas_out, xyz_out, dirs_out, ray_idx_out,
                     src_row_out);
  return check_launch("packed_resample_write (park)");
}
