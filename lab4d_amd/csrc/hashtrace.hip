// Sphere tracing of the hash field's SDF: one surface hit per ray.  Contract: include/lab4d_hashtrace.h; every rule and all of the arithmetic:
// hashtrace_math.hpp, shared with the CPU twin tests/host_harness/hashtrace/hashtrace_host.cpp.  The hot loop is the evaluator of
// k_hashsdf_fwd without its second table walk: the gather of 8 vertices per level and the 32 -> 64 -> 1 net per lane, repeated with a
// per-lane trip count.  Gather-bound, no MFMA.  No atomics, no read-back, no allocation: capturable in a hipGraph.
#include "common.hpp"
#include "hashtrace_math.hpp"

namespace lab4d {
namespace tr = lab4d_trace;
namespace hs = lab4d_hsdf;

// One lane per ray, grid-stride.  W1 | b1 | w2 in LDS (8.5 KB, read as broadcasts, as in k_hashsdf_fwd).  A lane leaves the loop when its ray
// ends; the wave goes on until its last lane has.  Across an evaluation a lane keeps the ray (o, d: 6), the bracket, the exit and len (4), the
// counters and the result: some 20 registers beside the 32 of enc.  trace_ray evaluates at ONE place per trip, so the gather and
// the net exist once in the code and lanes that step and lanes that bisect run them together.
template <int F>
__global__ void __launch_bounds__(tr::kBlock, 3) k_hashsdf_trace(const float* __restrict__ origin, const float* __restrict__ dir, const float* __restrict__ t_range,
                                                                const float* __restrict__ aabb_, long R, const float* __restrict__ table,
                                                                const int* __restrict__ res_, int log2_T_, const float* __restrict__ W1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                                tr::Params q, float* __restrict__ t_hit, int* __restrict__ status, int* __restrict__ n_eval,
                                                                float* __restrict__ sdf_hit) {
  __shared__ float s_W1[hs::kHid * hs::kEnc], s_b1[hs::kHid], s_w2[hs::kHid];
  for (int i = threadIdx.x; i < hs::kHid * hs::kEnc; i += blockDim.x) s_W1[i] = W1[i];
  if (threadIdx.x < hs::kHid) s_b1[threadIdx.x] = b1[threadIdx.x], s_w2[threadIdx.x] = w2[threadIdx.x];
  __syncthreads();
  const float bias2 = b2[0];
  const float aabb[6] = {aabb_[0], aabb_[1], aabb_[2], aabb_[3], aabb_[4], aabb_[5]};
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    const float o[3] = {origin[3 * r], origin[3 * r + 1], origin[3 * r + 2]};
    const float d[3] = {dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    const tr::Hit h = tr::trace_ray(o, d, t_range[2 * r], t_range[2 * r + 1], aabb, q, [&](const float* x01) {
      // (the per-level scalars are recomputed every evaluation instead of being hoisted out of the loop for all levels: see hashsdf.hip)
      const int* res = res_;
      int log2_T = log2_T_;
      asm volatile("" : "+s"(res), "+s"(log2_T));
      return tr::sdf_at<F>(x01, table, res, log2_T, s_W1, s_b1, s_w2, bias2);
    });
    t_hit[r] = h.t;
    status[r] = h.status;
    n_eval[r] = h.n_eval;
    sdf_hit[r] = h.sdf;
  }
}

}  // namespace lab4d
using namespace lab4d;

extern "C" int lab4d_hashsdf_trace(const float* origin, const float* dir, const float* t_range, const float* aabb, long R, const float* table,
                                   const int32_t* res, int L, int log2_T, int F, const float* W1, const float* b1, const float* w2, const float* b2,
                                   float eps, float step_scale, float min_step, int max_steps, int n_bisect, float* t_hit, int32_t* status,
                                   int32_t* n_eval, float* sdf_hit, void* stream) {
  LAB4D_REQUIRE(R >= 0 && R < (1L << 31), "hashsdf_trace: R = %ld outside [0, 2^31)", R);
  LAB4D_REQUIRE(L >= 1 && L <= 32 && F >= 1 && F <= 8 && L * F == lab4d_hsdf::kEnc,
                "hashsdf_trace: L = %d, F = %d: the geometry net is instantiated for L * F = 32 hash features (L <= 32, F <= 8)", L, F);
  LAB4D_REQUIRE(log2_T >= 4 && log2_T <= 24, "hashsdf_trace: log2_T = %d outside [4, 24]", log2_T);
  LAB4D_REQUIRE(lab4d_rn::finite_f(eps) && eps > 0.f, "hashsdf_trace: eps = %g must be finite and > 0", (double)eps);
  LAB4D_REQUIRE(step_scale > 0.f && step_scale <= 1.f, "hashsdf_trace: step_scale = %g outside (0, 1]", (double)step_scale);
  LAB4D_REQUIRE(lab4d_rn::finite_f(min_step) && min_step > 0.f, "hashsdf_trace: min_step = %g must be finite and > 0", (double)min_step);
  LAB4D_REQUIRE(max_steps >= 1 && max_steps <= tr::kMaxSteps, "hashsdf_trace: max_steps = %d outside [1, %d]", max_steps, tr::kMaxSteps);
  LAB4D_REQUIRE(n_bisect >= 0 && n_bisect <= tr::kMaxBisect, "hashsdf_trace: n_bisect = %d outside [0, %d]", n_bisect, tr::kMaxBisect);
  LAB4D_REQUIRE(aabb && table && res, "hashsdf_trace: null pointer (aabb, table, res)");
  LAB4D_REQUIRE(W1 && b1 && w2 && b2, "hashsdf_trace: null pointer (W1, b1, w2, b2)");
  if (R == 0) return LAB4D_OK;  // (the per-ray arrays are empty: an empty tensor's pointer is NULL)
  LAB4D_REQUIRE(origin && dir && t_range, "hashsdf_trace: null pointer (origin, dir, t_range)");
  LAB4D_REQUIRE(t_hit && status && n_eval && sdf_hit, "hashsdf_trace: null pointer (t_hit, status, n_eval, sdf_hit)");
  const tr::Params q = {eps, step_scale, min_step, max_steps, n_bisect};
  const int g = grid_1d(R, tr::kBlock, 2048);
#define LAUNCH_TRACE(FF)                                                                                                                              \
  hipLaunchKernelGGL(k_hashsdf_trace<FF>, dim3((unsigned)g), dim3(tr::kBlock), 0, (hipStream_t)stream, origin, dir, t_range, aabb, R, table, res, log2_T, W1, \
                     b1, w2, b2, q, t_hit, status, n_eval, sdf_hit)
  if (F == 1) LAUNCH_TRACE(1);
  else if (F == 2) LAUNCH_TRACE(2);
  else if (F == 4) LAUNCH_TRACE(4);
  else LAUNCH_TRACE(8);
#undef LAUNCH_TRACE
  return check_launch("hashsdf_trace");
}
