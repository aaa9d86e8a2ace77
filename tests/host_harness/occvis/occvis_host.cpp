// CPU twin of lab4d_amd/csrc/occvis.hip: serial loops over the SAME functions (csrc/occvis_math.hpp over csrc/occgrid_math.hpp) with the
// layout of include/lab4d_occvis.h.  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_occvis_host.py pins it against the
// rule in numpy float64 (tests/occvis_checks.py), the GPU suite holds the kernels word for word to it
// (tests/test_gpu_zzzzzzzzzzzzzzzzzoccvis.py).
#include <stdint.h>

#include "occvis_math.hpp"

namespace occ = lab4d_occ;
namespace occv = lab4d_occvis;

// sees (K, G^3, M) uint8: SEES per (cell, view), what the float64 rule is compared with
extern "C" void occvis_host_sees(const float* planes, int M, const float* aabbs, int K, int G, uint8_t* sees) {
  const long n = occ::n_cells(G);
  for (int lv = 0; lv < K; ++lv)
    for (long idx = 0; idx < n; ++idx) {
      float c[3], h[3], q[3];
      occv::cell_box(idx, aabbs + 6 * lv, G, c, h, q);
      for (int m = 0; m < M; ++m)
        sees[((long)lv * n + idx) * M + m] = occv::view_finite(planes + 24 * m) && occv::view_sees(planes + 24 * m, c, h, q) ? 1 : 0;
    }
}

// vis_bits (K, n_words(G)), n_visible (K): VISIBLE, every word rewritten
extern "C" void occvis_host_mark(const float* planes, int M, const float* aabbs, int K, int G, int min_views, uint32_t* vis_bits, int32_t* n_visible) {
  const long n = occ::n_cells(G), nw = occ::n_words(G);
  uint8_t* valid = new uint8_t[M];
  for (int m = 0; m < M; ++m) valid[m] = occv::view_finite(planes + 24 * m) ? 1 : 0;
  for (int lv = 0; lv < K; ++lv) {
    uint32_t* words = vis_bits + lv * nw;
    for (long w = 0; w < nw; ++w) words[w] = 0u;
    int32_t total = 0;
    for (long idx = 0; idx < n; ++idx) {
      float c[3], h[3], q[3];
      occv::cell_box(idx, aabbs + 6 * lv, G, c, h, q);
      int seen = 0;
      for (int m = 0; m < M && seen < min_views; ++m)
        if (valid[m] && occv::view_sees(planes + 24 * m, c, h, q)) ++seen;
      if (seen >= min_views) {
        words[idx >> 5] |= 1u << (idx & 31);
        ++total;
      }
    }
    n_visible[lv] = total;
  }
  delete[] valid;
}

// APPLY on K levels, in place on ema (K, G^3) and bits (K, n_words(G)); n_occupied (K) overwritten
extern "C" void occvis_host_apply(const uint32_t* vis_bits, float* ema, uint32_t* bits, int32_t* n_occupied, int K, int G) {
  const long n = occ::n_cells(G), nw = occ::n_words(G);
  for (int lv = 0; lv < K; ++lv) {
    int32_t total = 0;
    for (long idx = 0; idx < n; ++idx) {
      const bool on = occv::apply_cell(occ::bit_of(bits + lv * nw, idx), occ::bit_of(vis_bits + lv * nw, idx), &ema[lv * n + idx]);
      if (on) {
        ++total;
      } else {
        bits[lv * nw + (idx >> 5)] &= ~(1u << (idx & 31));
      }
    }
    n_occupied[lv] = total;
  }
}
