// Proposal (interval) loss between two packed sample lists per ray, and the adjoint of the compositing weights of a packed list.  Contract:
// include/lab4d_proposal.h; every rule: proposal_math.hpp (over presample_math.hpp, pmerge_math.hpp, prune_math.hpp and packed_math.hpp),
// shared with the CPU twin tests/host_harness/proposal/proposal_host.cpp, to which the envelope, forward and backward kernels are held word
// for word.  The partition is k_packed_composite_fwd's: one 64-lane wave per ray, four rays per 256-thread block, grid-stride.  The wave's
// index goes through readfirstlane, so the ray, its (start, count) in both lists, dir and every loop bound live in scalar registers and the
// shuffles run with all 64 lanes; in the backward kernel the fine rows' span and coef, which the whole wave reads at the same address, are
// scalar loads (written by an EARLIER launch: the scalar cache is clean at the start of a kernel).  No LDS, no atomics, vector stores only;
// nothing reads back or allocates: every entry point can be captured in a hipGraph.
#include "common.hpp"
#include "proposal_math.hpp"

namespace lab4d {
namespace pk = lab4d_packed;
namespace pp = lab4d_proposal;

__device__ __forceinline__ long first_ray() { return (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Two passes over the ray's rows: the first leaves S (the sum of g_w * w) and the ray's whole tau, the second recomputes tau, E and w 64 rows
// at a time with both carries and writes g_density.
__global__ void __launch_bounds__(256) k_packed_weights_bwd(const float* __restrict__ density, const float* __restrict__ deltas,
                                                             const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count, long R, long P,
                                                             const float* __restrict__ g_w, const float* __restrict__ g_trans, float* __restrict__ g_density) {
  const int lane = threadIdx.x & 63;
  for (long ray = first_ray(); ray < R; ray += (long)gridDim.x * 4) {
    const pp::Rows rr = pp::rows_of(ray_start, ray_count, ray, P);
    float S = 0.f, tail = 0.f;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
      float carry = 0.f, carry_s = 0.f;
      for (int j0 = 0; j0 < rr.n; j0 += 64) {
        const bool live = j0 + lane < rr.n;
        const long row = rr.s + j0 + lane;
        const float dens = live ? density[row] : 0.f, dl = live ? deltas[row] : 0.f, gw = live ? g_w[row] : 0.f;
        const float tau = pp::tau_of(dens, dl);
        const float incl = wave_scan_incl(tau, lane) + carry;
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = carry;
        carry = __shfl(incl, 63, 64);
        const float s_incl = wave_scan_incl(live ? pp::mul_rn(gw, pk::weight_of(tau, excl)) : 0.f, lane) + carry_s;
        carry_s = __shfl(s_incl, 63, 64);
        if (pass == 1 && live) g_density[row] = pp::g_density_of(pp::g_tau_of(gw, tau, excl, S, s_incl, tail), dens, dl);
      }
      S = carry_s;
      if (g_trans) tail = pp::mul_rn(g_trans[ray], pk::transmit_of(carry));
    }
  }
}

__global__ void __launch_bounds__(256) k_packed_envelope(const float* __restrict__ w_e, const float* __restrict__ t_e, const float* __restrict__ deltas_e,
                                                          const int32_t* __restrict__ ray_start_e, const int32_t* __restrict__ ray_count_e,
                                                          const float* __restrict__ dir, long R, long Pe, float* __restrict__ lo_e, float* __restrict__ hi_e,
                                                          float* __restrict__ cdf_e) {
  const int lane = threadIdx.x & 63;
  for (long ray = first_ray(); ray < R; ray += (long)gridDim.x * 4) {
    const pp::Rows rr = pp::rows_of(ray_start_e, ray_count_e, ray, Pe);
    if (rr.n == 0) continue;
    const float d[3] = {dir[3 * ray], dir[3 * ray + 1], dir[3 * ray + 2]};
    const float len = pk::dir_length(d);
    float carry = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      const float incl = wave_scan_incl(live ? pp::pos_of(w_e[row]) : 0.f, lane) + carry;
      carry = __shfl(incl, 63, 64);
      if (live) {
        const float t = t_e[row], h = pp::half_of(deltas_e[row], len);
        lo_e[row] = pp::lo_of(t, h);
        hi_e[row] = pp::hi_of(t, h);
        cdf_e[row] = incl;
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_packed_proposal_fwd(const float* __restrict__ lo_e, const float* __restrict__ hi_e, const float* __restrict__ cdf_e,
                                                              const int32_t* __restrict__ ray_start_e, const int32_t* __restrict__ ray_count_e, long Pe,
                                                              const float* __restrict__ w_f, const float* __restrict__ t_f, const float* __restrict__ deltas_f,
                                                              const int32_t* __restrict__ ray_start_f, const int32_t* __restrict__ ray_count_f, long Pf,
                                                              const float* __restrict__ dir, long R, float eps, int32_t* __restrict__ span,
                                                              float* __restrict__ coef, float* __restrict__ loss) {
  const int lane = threadIdx.x & 63;
  for (long ray = first_ray(); ray < R; ray += (long)gridDim.x * 4) {
    const pp::Rows re = pp::rows_of(ray_start_e, ray_count_e, ray, Pe);
    const pp::Rows rf = pp::rows_of(ray_start_f, ray_count_f, ray, Pf);
    float carry = 0.f;
    if (rf.n > 0) {
      const float d[3] = {dir[3 * ray], dir[3 * ray + 1], dir[3 * ray + 2]};
      const float len = pk::dir_length(d);
      for (int i0 = 0; i0 < rf.n; i0 += 64) {
        const bool live = i0 + lane < rf.n;
        const long row = rf.s + i0 + lane;
        float l = 0.f;
        if (live) {
          const float t = t_f[row], h = pp::half_of(deltas_f[row], len);
          const pp::Span sp = pp::span_of(lo_e + re.s, hi_e + re.s, re.n, pp::lo_of(t, h), pp::hi_of(t, h));
          const float v = pp::pos_of(w_f[row]);
          const float x = pp::excess_of(v, pp::bound_of(cdf_e + re.s, sp));
          l = pp::loss_of(x, v, eps);
          span[2 * row] = sp.j0;
          span[2 * row + 1] = sp.j1;
          coef[row] = pp::coef_of(x, v, eps);
        }
        const float incl = wave_scan_incl(l, lane) + carry;
        carry = __shfl(incl, 63, 64);
      }
    }
    if (lane == 0) loss[ray] = carry;
  }
}

// lanes over the ray's envelope rows 64 at a time; inside, the wave walks the ray's fine rows in ascending order: n_f * ceil(n_e / 64) steps
__global__ void __launch_bounds__(256) k_packed_proposal_bwd(const float* __restrict__ g_loss, const int32_t* __restrict__ span, const float* __restrict__ coef,
                                                              const float* __restrict__ w_e, const int32_t* __restrict__ ray_start_e,
                                                              const int32_t* __restrict__ ray_count_e, long Pe, const int32_t* __restrict__ ray_start_f,
                                                              const int32_t* __restrict__ ray_count_f, long Pf, long R, float* __restrict__ g_w_e) {
  const int lane = threadIdx.x & 63;
  for (long ray = first_ray(); ray < R; ray += (long)gridDim.x * 4) {
    const pp::Rows re = pp::rows_of(ray_start_e, ray_count_e, ray, Pe);
    const pp::Rows rf = pp::rows_of(ray_start_f, ray_count_f, ray, Pf);
    if (re.n == 0) continue;
    const float g = g_loss[ray];
    for (int j0 = 0; j0 < re.n; j0 += 64) {
      const int j = j0 + lane;
      float acc = 0.f;
      for (int i = 0; i < rf.n; ++i) acc = pp::accumulate(acc, g, coef[rf.s + i], j, span[2 * (rf.s + i)], span[2 * (rf.s + i) + 1]);
      if (j < re.n) g_w_e[re.s + j] = pp::gate(w_e[re.s + j], acc);
    }
  }
}

}  // namespace lab4d
using namespace lab4d;

static int check_rows(const char* what, long R, const char* pname, long P) {
  LAB4D_REQUIRE(R >= 0 && R < (1L << 31) && P >= 0 && P < (1L << 31), "%s: R = %ld or %s = %ld outside [0, 2^31)", what, R, pname, P);
  return LAB4D_OK;
}

extern "C" int lab4d_packed_weights_backward(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P,
                                             const float* g_w, const float* g_trans, float* g_density, void* stream) {
  if (int e = check_rows("packed_weights_backward", R, "P", P)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start && ray_count, "packed_weights_backward: null ray_start / ray_count");
  LAB4D_REQUIRE(P == 0 || (density && deltas && g_w && g_density), "packed_weights_backward: null density / deltas / g_w / g_density");
  if (P == 0) return LAB4D_OK;
  hipLaunchKernelGGL(k_packed_weights_bwd, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, density, deltas, ray_start, ray_count, R, P, g_w, g_trans,
                     g_density);
  return check_launch("packed_weights_backward");
}

extern "C" int lab4d_packed_envelope(const float* w_e, const float* t_e, const float* deltas_e, const int32_t* ray_start_e, const int32_t* ray_count_e,
                                     const float* dir, long R, long Pe, float* lo_e, float* hi_e, float* cdf_e, void* stream) {
  if (int e = check_rows("packed_envelope", R, "Pe", Pe)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start_e && ray_count_e && dir, "packed_envelope: null ray_start_e / ray_count_e / dir");
  LAB4D_REQUIRE(Pe == 0 || (w_e && t_e && deltas_e && lo_e && hi_e && cdf_e), "packed_envelope: null w_e / t_e / deltas_e / lo_e / hi_e / cdf_e");
  if (Pe == 0) return LAB4D_OK;
  hipLaunchKernelGGL(k_packed_envelope, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, w_e, t_e, deltas_e, ray_start_e, ray_count_e, dir, R, Pe, lo_e,
                     hi_e, cdf_e);
  return check_launch("packed_envelope");
}

extern "C" int lab4d_packed_proposal_forward(const float* lo_e, const float* hi_e, const float* cdf_e, const int32_t* ray_start_e, const int32_t* ray_count_e,
                                             long Pe, const float* w_f, const float* t_f, const float* deltas_f, const int32_t* ray_start_f,
                                             const int32_t* ray_count_f, long Pf, const float* dir, long R, float eps, int32_t* span, float* coef, float* loss,
                                             void* stream) {
  if (int e = check_rows("packed_proposal_forward", R, "Pe", Pe)) return e;
  if (int e = check_rows("packed_proposal_forward", R, "Pf", Pf)) return e;
  LAB4D_REQUIRE(eps >= 0.f && lab4d_rn::finite_f(eps), "packed_proposal_forward: eps = %g must be finite and >= 0", (double)eps);  // (NaN compares false)
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start_e && ray_count_e && ray_start_f && ray_count_f && dir && loss, "packed_proposal_forward: null per-ray pointer");
  LAB4D_REQUIRE(Pe == 0 || (lo_e && hi_e && cdf_e), "packed_proposal_forward: null lo_e / hi_e / cdf_e");
  LAB4D_REQUIRE(Pf == 0 || (w_f && t_f && deltas_f && span && coef), "packed_proposal_forward: null w_f / t_f / deltas_f / span / coef");
  hipLaunchKernelGGL(k_packed_proposal_fwd, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, lo_e, hi_e, cdf_e, ray_start_e, ray_count_e, Pe, w_f, t_f,
                     deltas_f, ray_start_f, ray_count_f, Pf, dir, R, eps, span, coef, loss);
  return check_launch("packed_proposal_forward");
}

extern "C" int lab4d_packed_proposal_backward(const float* g_loss, const int32_t* span, const float* coef, const float* w_e, const int32_t* ray_start_e,
                                              const int32_t* ray_count_e, long Pe, const int32_t* ray_start_f, const int32_t* ray_count_f, long Pf, long R,
                                              float* g_w_e, void* stream) {
  if (int e = check_rows("packed_proposal_backward", R, "Pe", Pe)) return e;
  if (int e = check_rows("packed_proposal_backward", R, "Pf", Pf)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(g_loss && ray_start_e && ray_count_e && ray_start_f && ray_count_f, "packed_proposal_backward: null per-ray pointer");
  LAB4D_REQUIRE(Pe == 0 || (w_e && g_w_e), "packed_proposal_backward: null w_e / g_w_e");
  LAB4D_REQUIRE(Pf == 0 || (span && coef), "packed_proposal_backward: null span / coef");
  if (Pe == 0) return LAB4D_OK;
  hipLaunchKernelGGL(k_packed_proposal_bwd, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, g_loss, span, coef, w_e, ray_start_e, ray_count_e, Pe,
                     ray_start_f, ray_count_f, Pf, R, g_w_e);
  return check_launch("packed_proposal_backward");
}
