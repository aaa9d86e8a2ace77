// CPU twin of lab4d_amd/csrc/presample.hip: serial loops over the SAME functions (csrc/presample_math.hpp over csrc/pmerge_math.hpp,
// csrc/prune_math.hpp and csrc/packed_math.hpp) with the layout of include/lab4d_presample.h.  A wave is emulated as 64 array entries: the
// doubling scans of wave_scan_incl (common.hpp) and wave_scan_max (presample.hip) step by step.  Built by tests/host_twin.py with
// g++ -ffp-contract=off; tests/test_presample_host.py pins it against the rules restated with numpy, the GPU suite holds both resample
// kernels word for word to it (tests/test_gpu_zzzzzzzzzzzzzzpresample.py).  presample_host_weights calls the host's expf: the kernel is held
// to float64, not to this function.
#include <stdint.h>

#include "presample_math.hpp"

namespace pk = lab4d_packed;
namespace ps = lab4d_presample;

// wave_scan_incl over all 64 lanes at once: every step reads the values of the step before
static void scan_incl(float* v) {
  for (int o = 1; o < 64; o <<= 1) {
    float before[64];
    for (int l = 0; l < 64; ++l) before[l] = v[l];
    for (int l = o; l < 64; ++l) v[l] = before[l] + before[l - o];
  }
}

// wave_scan_max likewise
static void scan_max(float* v) {
  for (int o = 1; o < 64; o <<= 1) {
    float before[64];
    for (int l = 0; l < 64; ++l) before[l] = v[l];
    for (int l = o; l < 64; ++l) v[l] = ps::later_of(before[l - o], before[l]);
  }
}

// w (P): rows of no ray are left as they are; trans (R) or NULL
extern "C" void presample_host_weights(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P, float* w,
                                       float* trans) {
  for (long ray = 0; ray < R; ++ray) {
    const ps::Rows rr = ps::rows_of(ray_start, ray_count, ray, P);
    float carry = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      float tau[64], incl[64];
      for (int l = 0; l < 64; ++l) incl[l] = tau[l] = j0 + l < rr.n ? ps::tau_of(density[rr.s + j0 + l], deltas[rr.s + j0 + l]) : 0.f;
      scan_incl(incl);
      for (int l = 0; l < 64; ++l) incl[l] += carry;
      for (int l = 0; l < 64 && j0 + l < rr.n; ++l) w[rr.s + j0 + l] = pk::weight_of(tau[l], l == 0 ? carry : incl[l - 1]);
      carry = incl[63];
    }
    if (trans) trans[ray] = pk::transmit_of(carry);
  }
}

// cdf (P): rows of no ray are left as they are
extern "C" void presample_host_count(const float* weights, const int32_t* ray_start, const int32_t* ray_count, long R, long P, int n_imp, float eps, float* cdf,
                                     float* mass, int32_t* new_count) {
  for (long ray = 0; ray < R; ++ray) {
    const ps::Rows rr = ps::rows_of(ray_start, ray_count, ray, P);
    float carry = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      float incl[64];
      for (int l = 0; l < 64; ++l) incl[l] = j0 + l < rr.n ? ps::mass_of(weights[rr.s + j0 + l], eps) : 0.f;
      scan_incl(incl);
      for (int l = 0; l < 64; ++l) incl[l] += carry;
      for (int l = 0; l < 64 && j0 + l < rr.n; ++l) cdf[rr.s + j0 + l] = incl[l];
      carry = incl[63];
    }
    mass[ray] = carry;
    new_count[ray] = ps::count_of(rr.n, carry, n_imp);
  }
}

// new_start: the exclusive prefix sum of presample_host_count's counts
extern "C" void presample_host_write(const float* weights, const float* cdf, const float* mass, const float* t, const float* deltas, const int32_t* ray_start,
                                     const int32_t* ray_count, const int32_t* new_start, long R, long P, const float* origin, const float* dir, const float* u,
                                     int n_imp, float eps, long cap, const float* aabb, float* t_out, float* deltas_out, float* xyz_out, float* dirs_out,
                                     int32_t* ray_idx_out, int32_t* src_row_out, int32_t* new_count_out, int32_t* total, uint8_t* overflow) {
  long tot = 0;
  for (long ray = 0; ray < R; ++ray) {
    const ps::Rows rr = ps::rows_of(ray_start, ray_count, ray, P);
    const long base = new_start[ray];
    const float W = mass[ray];
    const int n = ps::count_of(rr.n, W, n_imp);
    if (n > 0) {
      const float* o = origin + 3 * ray;
      const float* d = dir + 3 * ray;
      const float len = pk::dir_length(d);
      const float* C = cdf + rr.s;
      float carry = -lab4d_rn::inf_f();
      for (int k0 = 0; k0 < n; k0 += 64) {
        float tk[64], span[64];
        long row[64];
        for (int l = 0; l < 64; ++l) {
          const int k = k0 + l;
          tk[l] = -lab4d_rn::inf_f(), span[l] = 0.f, row[l] = 0;
          if (k >= n) continue;
          const float q = ps::mul_rn(u ? ps::clamp01(u[ray * n_imp + k]) : ps::query_u(k, n_imp), W);
          const int i = ps::row_of(C, rr.n, q);
          row[l] = rr.s + i;
          const float m = ps::mass_of(weights[row[l]], eps), dl = deltas[row[l]];
          tk[l] = ps::t_of(t[row[l]], ps::place_f(q, i > 0 ? C[i - 1] : 0.f, m), ps::width_of(dl, len));
          span[l] = ps::span_of(dl, W, n_imp, m);
        }
        scan_max(tk);
        for (int l = 0; l < 64; ++l) tk[l] = ps::later_of(carry, tk[l]);
        carry = tk[63];
        for (int l = 0; l < 64 && k0 + l < n; ++l) {
          const long dst = base + k0 + l;
          if (dst < 0 || dst >= cap) continue;
          float p[3];
          pk::point_at(o, d, tk[l], p);
          t_out[dst] = tk[l];
          deltas_out[dst] = span[l];
          for (int a = 0; a < 3; ++a) {
            xyz_out[3 * dst + a] = p[a];
            dirs_out[3 * dst + a] = len > 0.f ? ps::div_rn(d[a], len) : 0.f;
          }
          ray_idx_out[dst] = (int32_t)ray;
          src_row_out[dst] = (int32_t)row[l];
        }
      }
    }
    new_count_out[ray] = pk::clamp_count((int)base, n, (int)cap);
    tot = base + n;
  }
  *total = (int32_t)tot;
  *overflow = tot > cap ? 1 : 0;
  float p[3];
  pk::park_point(aabb, p);
  for (long row = tot < 0 ? 0 : tot; row < cap; ++row) {
    t_out[row] = 0.f;
    deltas_out[row] = 0.f;
    for (int a = 0; a < 3; ++a) {
      xyz_out[3 * row + a] = p[a];
      dirs_out[3 * row + a] = a == 2 ? 1.f : 0.f;
    }
    ray_idx_out[row] = -1;
    src_row_out[row] = -1;
  }
}
