// CPU twin of lab4d_amd/csrc/conemarch.hip: serial loops over the SAME functions (csrc/conemarch_math.hpp over csrc/occgrid_math.hpp and
// csrc/ray_math.hpp) with the layout of include/lab4d_conemarch.h.  Built by tests/host_twin.py with g++ -ffp-contract=off;
// tests/test_conemarch_host.py pins it against a numpy float32 restatement of the rules word for word, the GPU suite holds the kernels word
// for word to it (tests/test_gpu_zzzzzzzzzzzzzzzzconemarch.py).
#include <stdint.h>

#include "conemarch_math.hpp"

namespace occ = lab4d_occ;
namespace cone = lab4d_cone;

// delta, level: may be null (delta = 0 for every point)
extern "C" void conemarch_host_cascade_mask(const float* xyz, const float* delta, const float* aabbs, const uint32_t* bits, int K, int G, long S,
                                            uint8_t* mask, int32_t* level) {
  const cone::Edges E = cone::cascade_edges(aabbs, K, G);
  for (long s = 0; s < S; ++s) {
    int lv;
    mask[s] = cone::cascade_keep(xyz + 3 * s, delta ? delta[s] : 0.f, aabbs, bits, E, K, G, &lv) ? 1 : 0;
    if (level) level[s] = lv;
  }
}

extern "C" void conemarch_host_count(const float* origin, const float* dir, const float* t_range, const float* aabbs, const uint32_t* bits, int K, int G,
                                     long R, float cone_angle, float dt_min, float dt_max, int k_max, int32_t* ray_count) {
  const cone::Edges E = cone::cascade_edges(aabbs, K, G);
  for (long r = 0; r < R; ++r)
    ray_count[r] = cone::march_cone_ray(origin + 3 * r, dir + 3 * r, t_range[2 * r], t_range[2 * r + 1], aabbs, bits, E, K, G, cone_angle, dt_min, dt_max,
                                        k_max, [](int, float, float, float, const float*, int) {});
}

// ray_start: the exclusive prefix sum of conemarch_host_count's counts
extern "C" void conemarch_host_write(const float* origin, const float* dir, const float* t_range, const float* aabbs, const uint32_t* bits, int K, int G,
                                     long R, float cone_angle, float dt_min, float dt_max, int k_max, const int32_t* ray_start, long cap, float* t_out,
                                     float* steps, float* deltas, float* xyz, float* dirs, int32_t* ray_idx, int32_t* level, int32_t* ray_count_out,
                                     int32_t* total, uint8_t* overflow) {
  const cone::Edges E = cone::cascade_edges(aabbs, K, G);
  long tot = 0;
  for (long r = 0; r < R; ++r) {
    const float* d = dir + 3 * r;
    const float len = cone::dir_length(d);
    float u[3];
    for (int a = 0; a < 3; ++a) u[a] = len > 0.f ? occ::div_rn(d[a], len) : 0.f;
    const long start = ray_start[r];
    const int n = cone::march_cone_ray(origin + 3 * r, d, t_range[2 * r], t_range[2 * r + 1], aabbs, bits, E, K, G, cone_angle, dt_min, dt_max, k_max,
                                       [&](int i, float t, float s, float delta, const float* p, int lv) {
      const long row = start + i;
      if (row < 0 || row >= cap) return;
      t_out[row] = t;
      steps[row] = s;
      deltas[row] = delta;
      for (int a = 0; a < 3; ++a) {
        xyz[3 * row + a] = p[a];
        dirs[3 * row + a] = u[a];
      }
      ray_idx[row] = (int32_t)r;
      level[row] = lv;
    });
    ray_count_out[r] = cone::clamp_count((int)start, n, (int)cap);
    tot = start + n;
  }
  *total = (int32_t)tot;
  *overflow = tot > cap ? 1 : 0;
  float p[3];
  cone::park_point(aabbs + 6 * (K - 1), p);
  for (long row = tot; row < cap; ++row) {
    t_out[row] = 0.f;
    steps[row] = 0.f;
    deltas[row] = 0.f;
    for (int a = 0; a < 3; ++a) {
      xyz[3 * row + a] = p[a];
      dirs[3 * row + a] = a == 2 ? 1.f : 0.f;
    }
    ray_idx[row] = -1;
    level[row] = -1;
  }
}
