// CPU twin of lab4d_amd/csrc/proposal.hip: serial loops over the SAME functions (csrc/proposal_math.hpp over csrc/presample_math.hpp,
// csrc/pmerge_math.hpp, csrc/prune_math.hpp and csrc/packed_math.hpp) with the layout of include/lab4d_proposal.h.  A wave is emulated as 64
// array entries: the doubling scan of wave_scan_incl (common.hpp) step by step.  Built by tests/host_twin.py with g++ -ffp-contract=off;
// tests/test_proposal_host.py pins it against the rules restated with numpy, the GPU suite holds the envelope, forward and backward kernels
// word for word to it (tests/test_gpu_zzzzzzzzzzzzzzzproposal.py).  proposal_host_weights_backward calls the host's expf: the kernel is held
// to float64, not to this function.
#include <stdint.h>

#include "proposal_math.hpp"

namespace pk = lab4d_packed;
namespace pp = lab4d_proposal;

// wave_scan_incl over all 64 lanes at once: every step reads the values of the step before
static void scan_incl(float* v) {
  for (int o = 1; o < 64; o <<= 1) {
    float before[64];
    for (int l = 0; l < 64; ++l) before[l] = v[l];
    for (int l = o; l < 64; ++l) v[l] = before[l] + before[l - o];
  }
}

// g_density (P): rows of no ray are left as they are; g_trans (R) or NULL
extern "C" void proposal_host_weights_backward(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P,
                                               const float* g_w, const float* g_trans, float* g_density) {
  for (long ray = 0; ray < R; ++ray) {
    const pp::Rows rr = pp::rows_of(ray_start, ray_count, ray, P);
    float S = 0.f, tail = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
      float carry = 0.f, carry_s = 0.f;
      for (int j0 = 0; j0 < rr.n; j0 += 64) {
        float tau[64], incl[64], s_incl[64];
        for (int l = 0; l < 64; ++l) incl[l] = tau[l] = j0 + l < rr.n ? pp::tau_of(density[rr.s + j0 + l], deltas[rr.s + j0 + l]) : 0.f;
        scan_incl(incl);
        for (int l = 0; l < 64; ++l) incl[l] += carry;
        for (int l = 0; l < 64; ++l)
          s_incl[l] = j0 + l < rr.n ? pp::mul_rn(g_w[rr.s + j0 + l], pk::weight_of(tau[l], l == 0 ? carry : incl[l - 1])) : 0.f;
        scan_incl(s_incl);
        for (int l = 0; l < 64; ++l) s_incl[l] += carry_s;
        for (int l = 0; pass == 1 && l < 64 && j0 + l < rr.n; ++l) {
          const long row = rr.s + j0 + l;
          g_density[row] = pp::g_density_of(pp::g_tau_of(g_w[row], tau[l], l == 0 ? carry : incl[l - 1], S, s_incl[l], tail), density[row], deltas[row]);
        }
        carry = incl[63];
        carry_s = s_incl[63];
      }
      S = carry_s;
      if (g_trans) tail = pp::mul_rn(g_trans[ray], pk::transmit_of(carry));
    }
  }
}

// lo_e, hi_e, cdf_e (Pe): rows of no ray are left as they are
extern "C" void proposal_host_envelope(const float* w_e, const float* t_e, const float* deltas_e, const int32_t* ray_start_e, const int32_t* ray_count_e,
                                       const float* dir, long R, long Pe, float* lo_e, float* hi_e, float* cdf_e) {
  for (long ray = 0; ray < R; ++ray) {
    const pp::Rows rr = pp::rows_of(ray_start_e, ray_count_e, ray, Pe);
    if (rr.n == 0) continue;
    const float len = pk::dir_length(dir + 3 * ray);
    float carry = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      float incl[64];
      for (int l = 0; l < 64; ++l) incl[l] = j0 + l < rr.n ? pp::pos_of(w_e[rr.s + j0 + l]) : 0.f;
      scan_incl(incl);
      for (int l = 0; l < 64; ++l) incl[l] += carry;
      for (int l = 0; l < 64 && j0 + l < rr.n; ++l) {
        const long row = rr.s + j0 + l;
        const float h = pp::half_of(deltas_e[row], len);
        lo_e[row] = pp::lo_of(t_e[row], h);
        hi_e[row] = pp::hi_of(t_e[row], h);
        cdf_e[row] = incl[l];
      }
      carry = incl[63];
    }
  }
}

// span (Pf, 2), coef (Pf): rows of no ray are left as they are; loss (R)
extern "C" void proposal_host_forward(const float* lo_e, const float* hi_e, const float* cdf_e, const int32_t* ray_start_e, const int32_t* ray_count_e, long Pe,
                                      const float* w_f, const float* t_f, const float* deltas_f, const int32_t* ray_start_f, const int32_t* ray_count_f, long Pf,
                                      const float* dir, long R, float eps, int32_t* span, float* coef, float* loss) {
  for (long ray = 0; ray < R; ++ray) {
    const pp::Rows re = pp::rows_of(ray_start_e, ray_count_e, ray, Pe);
    const pp::Rows rf = pp::rows_of(ray_start_f, ray_count_f, ray, Pf);
    float carry = 0.f;
    if (rf.n > 0) {
      const float len = pk::dir_length(dir + 3 * ray);
      for (int i0 = 0; i0 < rf.n; i0 += 64) {
        float incl[64];
        for (int l = 0; l < 64; ++l) {
          incl[l] = 0.f;
          if (i0 + l >= rf.n) continue;
          const long row = rf.s + i0 + l;
          const float h = pp::half_of(deltas_f[row], len);
          const pp::Span sp = pp::span_of(lo_e + re.s, hi_e + re.s, re.n, pp::lo_of(t_f[row], h), pp::hi_of(t_f[row], h));
          const float v = pp::pos_of(w_f[row]);
          const float x = pp::excess_of(v, pp::bound_of(cdf_e + re.s, sp));
          incl[l] = pp::loss_of(x, v, eps);
          span[2 * row] = sp.j0;
          span[2 * row + 1] = sp.j1;
          coef[row] = pp::coef_of(x, v, eps);
        }
        scan_incl(incl);
        carry = incl[63] + carry;
      }
    }
    loss[ray] = carry;
  }
}

// g_w_e (Pe): rows of no ray are left as they are
extern "C" void proposal_host_backward(const float* g_loss, const int32_t* span, const float* coef, const float* w_e, const int32_t* ray_start_e,
                                       const int32_t* ray_count_e, long Pe, const int32_t* ray_start_f, const int32_t* ray_count_f, long Pf, long R,
                                       float* g_w_e) {
  for (long ray = 0; ray < R; ++ray) {
    const pp::Rows re = pp::rows_of(ray_start_e, ray_count_e, ray, Pe);
    const pp::Rows rf = pp::rows_of(ray_start_f, ray_count_f, ray, Pf);
    for (int j = 0; j < re.n; ++j) {
      float acc = 0.f;
      for (int i = 0; i < rf.n; ++i) acc = pp::accumulate(acc, g_loss[ray], coef[rf.s + i], j, span[2 * (rf.s + i)], span[2 * (rf.s + i) + 1]);
      g_w_e[re.s + j] = pp::gate(w_e[re.s + j], acc);
    }
  }
}
