// CPU twin of lab4d_amd/csrc/distort.hip: serial loops over the SAME per-row functions (csrc/distort_math.hpp over csrc/prune_math.hpp and
// csrc/packed_math.hpp) with the layout of include/lab4d_distort.h.  Every prefix is a serial fp32 sum along the ray, so the sums run in
// another order than the kernels' chunked wave scans: the GPU suite holds the kernels to this twin within the fp32 bar, not word for word
// (tests/test_gpu_zzzzzzzzzdistort.py).  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_distort_host.py pins it against the
// float64 definition.
#include <stdint.h>

#include "distort_math.hpp"

namespace pk = lab4d_packed;
namespace ds = lab4d_distort;

// the ray's totals of w and w m, and its loss
static void ray_totals(const float* density, const float* deltas, const float* mid, const float* width, const ds::Rows rr, float* W_total, float* M_total,
                       float* loss) {
  float E = 0.f, W = 0.f, M = 0.f, l = 0.f;
  for (int i = 0; i < rr.n; ++i) {
    const long row = rr.s + i;
    const float tau = density[row] * deltas[row];
    const float w = pk::weight_of(tau, E), m = ds::shifted_mid(mid[row], mid[rr.s]);
    l += ds::pair_term(w, m, W, M) + ds::self_term(w, width[row]);
    E += tau;
    W += w;
    M += w * m;
  }
  *W_total = W, *M_total = M, *loss = l;
}

// loss (R): written for every ray
extern "C" void distort_host_forward(const float* density, const float* deltas, const float* mid, const float* width, const int32_t* ray_start,
                                     const int32_t* ray_count, long R, long P, float* loss) {
  for (long ray = 0; ray < R; ++ray) {
    float W, M;
    ray_totals(density, deltas, mid, width, ds::rows_of(ray_start, ray_count, ray, P), &W, &M, &loss[ray]);
  }
}

// g_density, g_deltas (P) or null: rows of no ray are left as they are
extern "C" void distort_host_backward(const float* density, const float* deltas, const float* mid, const float* width, const int32_t* ray_start,
                                      const int32_t* ray_count, long R, long P, const float* g_loss, float* g_density, float* g_deltas) {
  if (!g_density && !g_deltas) return;
  for (long ray = 0; ray < R; ++ray) {
    const ds::Rows rr = ds::rows_of(ray_start, ray_count, ray, P);
    if (rr.n == 0) continue;
    float W_total, M_total, loss;
    ray_totals(density, deltas, mid, width, rr, &W_total, &M_total, &loss);
    float E = 0.f, W = 0.f, M = 0.f, G = 0.f;
    for (int i = 0; i < rr.n; ++i) {
      const long row = rr.s + i;
      const float tau = density[row] * deltas[row];
      const float w = pk::weight_of(tau, E), m = ds::shifted_mid(mid[row], mid[rr.s]);
      const float W_incl = W + w, M_incl = M + w * m;
      const float gw = ds::weight_adjoint(w, m, width[row], W, M, W_incl, M_incl, W_total, M_total);
      E += tau;
      G += gw * w;
      const float gtau = g_loss[ray] * ds::tau_adjoint(gw, pk::transmit_of(E), ds::suffix_of(loss, G));
      if (g_density) g_density[row] = gtau * deltas[row];
      if (g_deltas) g_deltas[row] = gtau * density[row];
      W = W_incl, M = M_incl;
    }
  }
}
