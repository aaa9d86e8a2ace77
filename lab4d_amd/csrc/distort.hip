// Distortion loss of a packed sample list, forward and adjoint.  Contract: include/lab4d_distort.h; the per-row arithmetic: distort_math.hpp
// (over prune_math.hpp / packed_math.hpp), shared with the CPU twin tests/host_harness/distort/distort_host.cpp; the weights: chunk_weights of
// packed_chunk.hpp, the compositor's own.  The partition is k_packed_composite_fwd's: one 64-lane wave per ray, four rays per 256-thread
// block, grid-stride, lanes over the ray's consecutive rows 64 at a time, one wave scan with a carry per scanned quantity (tau, w, w m, and
// in the adjoint g_w w).  Every loop bound is the wave's own ray, so the shuffles run with all 64 lanes.  No LDS, no atomics, no scratch;
// nothing reads back or allocates: both entry points can be captured in a hipGraph.
#include "common.hpp"
#include "distort_math.hpp"
#include "packed_chunk.hpp"

namespace lab4d {
namespace ds = lab4d_distort;

struct Prefix {
  float excl, incl;
};
// the prefixes of v along the ray; carry: the sum over the chunks before this one on entry, this one included on exit
__device__ __forceinline__ Prefix chunk_prefix(float v, int lane, float& carry) {
  const float incl = wave_scan_incl(v, lane) + carry;
  float excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = carry;
  carry = __shfl(incl, 63, 64);
  return {excl, incl};
}

struct RayTotals {
  float W, M, loss;
};
// One forward sweep over a ray with rows (rr.n > 0): the totals of w and w m and the loss, the same value in every lane.
__device__ __forceinline__ RayTotals ray_totals(const float* __restrict__ density, const float* __restrict__ deltas, const float* __restrict__ mid,
                                                const float* __restrict__ width, const ds::Rows rr, float mid_first, int lane) {
  float c_tau = 0.f, c_w = 0.f, c_wm = 0.f, part = 0.f;
  for (int j0 = 0; j0 < rr.n; j0 += 64) {
    const bool live = j0 + lane < rr.n;
    const long row = rr.s + j0 + lane;
    const ChunkWeights cw = chunk_weights(density, deltas, row, live, lane, c_tau);
    const float m = live ? ds::shifted_mid(mid[row], mid_first) : 0.f;
    const float wd = live ? width[row] : 0.f;
    const Prefix W = chunk_prefix(cw.w, lane, c_w);
    const Prefix M = chunk_prefix(cw.w * m, lane, c_wm);
    part += ds::pair_term(cw.w, m, W.excl, M.excl) + ds::self_term(cw.w, wd);  // (0 in the lanes behind the ray: w = 0)
  }
  return {c_w, c_wm, wave_sum(part)};
}

__global__ void __launch_bounds__(256) k_packed_distortion_fwd(const float* __restrict__ density, const float* __restrict__ deltas,
                                                                const float* __restrict__ mid, const float* __restrict__ width,
                                                                const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count, long R, long P,
                                                                float* __restrict__ loss) {
  const int lane = threadIdx.x & 63;
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const ds::Rows rr = ds::rows_of(ray_start, ray_count, ray, P);
    float l = 0.f;
    if (rr.n > 0) l = ray_totals(density, deltas, mid, width, rr, mid[rr.s], lane).loss;
    if (lane == 0) loss[ray] = l;
  }
}

// Sweep 1 is the forward's; sweep 2 walks the ray forwards again with the totals in hand: S_i comes from 2 loss and the inclusive prefix of
// g_w w, so nothing runs backwards and nothing is parked in the gradient rows.
__global__ void __launch_bounds__(256) k_packed_distortion_bwd(const float* __restrict__ density, const float* __restrict__ deltas,
                                                                const float* __restrict__ mid, const float* __restrict__ width,
                                                                const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count, long R, long P,
                                                                const float* __restrict__ g_loss, float* __restrict__ g_density,
                                                                float* __restrict__ g_deltas) {
  const int lane = threadIdx.x & 63;
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const ds::Rows rr = ds::rows_of(ray_start, ray_count, ray, P);
    if (rr.n == 0) continue;
    const float gl = g_loss[ray], mid_first = mid[rr.s];
    const RayTotals tot = ray_totals(density, deltas, mid, width, rr, mid_first, lane);
    float c_tau = 0.f, c_w = 0.f, c_wm = 0.f, c_gww = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      const ChunkWeights cw = chunk_weights(density, deltas, row, live, lane, c_tau);
      const float m = live ? ds::shifted_mid(mid[row], mid_first) : 0.f;
      const float wd = live ? width[row] : 0.f;
      const Prefix W = chunk_prefix(cw.w, lane, c_w);
      const Prefix M = chunk_prefix(cw.w * m, lane, c_wm);
      const float gw = ds::weight_adjoint(cw.w, m, wd, W.excl, M.excl, W.incl, M.incl, tot.W, tot.M);
      const Prefix G = chunk_prefix(gw * cw.w, lane, c_gww);  // (0 in the lanes behind the ray: w = 0)
      const float gtau = gl * ds::tau_adjoint(gw, cw.T, ds::suffix_of(tot.loss, G.incl));
      if (live) {
        const float dn = density[row], dl = deltas[row];
        if (g_density) g_density[row] = gtau * dl;
        if (g_deltas) g_deltas[row] = gtau * dn;
      }
    }
  }
}

}  // namespace lab4d
using namespace lab4d;

static int check_rows(const char* what, long R, long P) {
  LAB4D_REQUIRE(R >= 0 && R < (1L << 31) && P >= 0 && P < (1L << 31), "%s: R = %ld or P = %ld outside [0, 2^31)", what, R, P);
  return LAB4D_OK;
}

extern "C" int lab4d_packed_distortion_forward(const float* density, const float* deltas, const float* mid, const float* width, const int32_t* ray_start,
                                               const int32_t* ray_count, long R, long P, float* loss, void* stream) {
  if (int e = check_rows("packed_distortion_forward", R, P)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start && ray_count && loss, "packed_distortion_forward: null ray_start / ray_count / loss");
  LAB4D_REQUIRE(P == 0 || (density && deltas && mid && width), "packed_distortion_forward: null density / deltas / mid / width");
  hipLaunchKernelGGL(k_packed_distortion_fwd, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, density, deltas, mid, width, ray_start, ray_count, R,
                     P, loss);
  return check_launch("packed_distortion_forward");
}

extern "C" int lab4d_packed_distortion_backward(const float* density, const float* deltas, const float* mid, const float* width, const int32_t* ray_start,
                                                const int32_t* ray_count, long R, long P, const float* g_loss, float* g_density, float* g_deltas,
                                                void* stream) {
  if (int e = check_rows("packed_distortion_backward", R, P)) return e;
  if (!g_density && !g_deltas) return LAB4D_OK;
  if (R == 0 || P == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start && ray_count && g_loss, "packed_distortion_backward: null ray_start / ray_count / g_loss");
  LAB4D_REQUIRE(density && deltas && mid && width, "packed_distortion_backward: null density / deltas / mid / width");
  hipLaunchKernelGGL(k_packed_distortion_bwd, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, density, deltas, mid, width, ray_start, ray_count, R,
                     P, g_loss, g_density, g_deltas);
  return check_launch("packed_distortion_backward");
}
