// CPU twin of lab4d_amd/csrc/occgrid.hip: serial loops over the SAME functions (csrc/occgrid_math.hpp) with the layout of
// include/lab4d_occgrid.h.  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_occgrid_host.py pins it against
// numpy in float64, the GPU suite holds the kernels bit for bit to it (tests/test_gpu_zzzzoccgrid.py).
#include <stdint.h>

#include "occgrid_math.hpp"

namespace occ = lab4d_occ;

// the state "nothing known yet": every bit of the grid set (padding bits of the last word zero), ema = +inf
extern "C" void occgrid_host_init(float* ema, uint32_t* bits, int32_t* n_occupied, int G) {
  const long n = occ::n_cells(G), nw = occ::n_words(G);
  for (long w = 0; w < nw; ++w) bits[w] = 0;
  for (long i = 0; i < n; ++i) {
    ema[i] = INFINITY;
    bits[i >> 5] |= 1u << (i & 31);
  }
  *n_occupied = (int32_t)n;
}

extern "C" void occgrid_host_update(const float* density, float* ema, uint32_t* bits, int32_t* n_occupied, int G, float decay, float thresh) {
  const long n = occ::n_cells(G), nw = occ::n_words(G);
  for (long w = 0; w < nw; ++w) bits[w] = 0;
  int32_t count = 0;
  for (long i = 0; i < n; ++i) {
    ema[i] = occ::ema_next(ema[i], density[i], decay);
    if (occ::occupied(ema[i], thresh)) {
      bits[i >> 5] |= 1u << (i & 31);
      ++count;
    }
  }
  *n_occupied = count;
}

extern "C" void occgrid_host_mask(const float* xyz, const float* aabb, const uint32_t* bits, int G, long S, uint8_t* mask) {
  for (long s = 0; s < S; ++s) mask[s] = occ::sample_mask(xyz + 3 * s, aabb, bits, G) ? 1 : 0;
}

// steps (R, may be null): cells the walk visited
extern "C" void occgrid_host_ray_span(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G, long R,
                                      float* t_span, uint8_t* hit, int32_t* steps) {
  for (long r = 0; r < R; ++r) {
    int n = 0;
    hit[r] = occ::ray_span(origin + 3 * r, dir + 3 * r, t_range[2 * r], t_range[2 * r + 1], aabb, bits, G, t_span + 2 * r, &n) ? 1 : 0;
    if (steps) steps[r] = n;
  }
}
