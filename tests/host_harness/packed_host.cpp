// CPU twin of lab4d_amd/csrc/packed.hip: serial loops over the SAME functions (csrc/packed_math.hpp over csrc/occgrid_math.hpp) with the
// layout of include/lab4d_packed.h.  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_packed_host.py pins it against
// numpy / torch in float64, the GPU suite holds the march kernels word for word to it (tests/test_gpu_zzzzzpacked.py).
#include <stdint.h>

#include <vector>

#include "packed_math.hpp"

namespace occ = lab4d_occ;
namespace pk = lab4d_packed;

extern "C" void packed_host_march_count(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G, long R,
                                        float dt, int k_max, int32_t* ray_count) {
  for (long r = 0; r < R; ++r)
    ray_count[r] = pk::march_ray(origin + 3 * r, dir + 3 * r, t_range[2 * r], t_range[2 * r + 1], aabb, bits, G, dt, k_max, [](int, float, const float*) {});
}

// ray_start: the exclusive prefix sum of packed_host_march_count's counts
extern "C" void packed_host_march_write(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G, long R,
                                        float dt, int k_max, const int32_t* ray_start, long cap, float* t_out, float* deltas, float* xyz, float* dirs,
                                        int32_t* ray_idx, int32_t* ray_count_out, int32_t* total, uint8_t* overflow) {
  long tot = 0;
  for (long r = 0; r < R; ++r) {
    const float* d = dir + 3 * r;
    const float len = pk::dir_length(d);
    float u[3];
    for (int a = 0; a < 3; ++a) u[a] = len > 0.f ? occ::div_rn(d[a], len) : 0.f;
    const float delta = occ::mul_rn(dt, len);
    const long start = ray_start[r];
    const int n = pk::march_ray(origin + 3 * r, d, t_range[2 * r], t_range[2 * r + 1], aabb, bits, G, dt, k_max, [&](int i, float t, const float* p) {
      const long row = start + i;
      if (row < 0 || row >= cap) return;
      t_out[row] = t;
      deltas[row] = delta;
      for (int a = 0; a < 3; ++a) {
        xyz[3 * row + a] = p[a];
        dirs[3 * row + a] = u[a];
      }
      ray_idx[row] = (int32_t)r;
    });
    ray_count_out[r] = pk::clamp_count((int)start, n, (int)cap);
    tot = start + n;
  }
  *total = (int32_t)tot;
  *overflow = tot > cap ? 1 : 0;
  float p[3];
  pk::park_point(aabb, p);
  for (long row = tot; row < cap; ++row) {
    t_out[row] = 0.f;
    deltas[row] = 0.f;
    for (int a = 0; a < 3; ++a) {
      xyz[3 * row + a] = p[a];
      dirs[3 * row + a] = a == 2 ? 1.f : 0.f;
    }
    ray_idx[row] = -1;
  }
}

static void rows_of(const int32_t* ray_start, const int32_t* ray_count, long ray, long P, long* s, long* n) {
  *s = ray_start[ray];
  *n = ray_count[ray];
  if (*s < 0 || *s >= P || *n <= 0) *s = *n = 0;
  if (*n > P - *s) *n = P - *s;
}

static int sum_channels(int n_fields, const int* channels, const int* modes) {
  int s = 0;
  for (int f = 0; f < n_fields; ++f) s += modes[f] == 2 ? 1 : channels[f];
  return s;
}

// weights / transmit (P, may be null), mask (R), out (R, sum channels)
extern "C" void packed_host_composite_forward(const float* density, const float* deltas, int n_fields, const float* const* fields, const int* channels,
                                              const int* modes, const int32_t* ray_start, const int32_t* ray_count, long R, long P, float* weights,
                                              float* transmit, float* mask, float* out) {
  const int sumC = sum_channels(n_fields, channels, modes);
  for (long ray = 0; ray < R; ++ray) {
    long s, n;
    rows_of(ray_start, ray_count, ray, P, &s, &n);
    std::vector<float> w(n);
    float cum = 0.f, msum = 0.f;
    for (long i = 0; i < n; ++i) {
      const float tau = density[s + i] * deltas[s + i];
      w[i] = pk::weight_of(tau, cum);
      cum += tau;
      if (weights) weights[s + i] = w[i];
      if (transmit) transmit[s + i] = pk::transmit_of(cum);
      msum += w[i];
    }
    mask[ray] = msum;
    const float inv = pk::normaliser(msum);
    int co = 0;
    for (int f = 0; f < n_fields; ++f) {
      const int C = channels[f];
      const float* v = fields[f] + s * C;
      if (modes[f] == 2) {
        float x = 0.f;
        for (long e = 0; e < n * C; ++e) x += v[e];
        out[ray * sumC + co] = n > 0 ? x / ((float)n * (float)C) : 0.f;
        co += 1;
      } else {
        for (int c = 0; c < C; ++c) {
          float x = 0.f;
          for (long i = 0; i < n; ++i) x += w[i] * v[i * C + c];
          out[ray * sumC + co + c] = x * inv;
        }
        co += C;
      }
    }
  }
}

// g_mask (R), g_out (R, sum channels): may be null.  g_density, g_deltas (P), g_fields[f] (P, c_f): may be null; rows of no ray are left alone.
extern "C" void packed_host_composite_backward(const float* density, const float* deltas, int n_fields, const float* const* fields, const int* channels,
                                               const int* modes, const int32_t* ray_start, const int32_t* ray_count, long R, long P, const float* g_mask,
                                               const float* g_out, float* g_density, float* g_deltas, float* const* g_fields) {
  const int sumC = sum_channels(n_fields, channels, modes);
  for (long ray = 0; ray < R; ++ray) {
    long s, n;
    rows_of(ray_start, ray_count, ray, P, &s, &n);
    if (n == 0) continue;
    std::vector<float> w(n), T(n), A(n, 0.f);
    float cum = 0.f, msum = 0.f;
    for (long i = 0; i < n; ++i) {
      const float tau = density[s + i] * deltas[s + i];
      w[i] = pk::weight_of(tau, cum);
      cum += tau;
      T[i] = pk::transmit_of(cum);
      msum += w[i];
    }
    const float inv = pk::normaliser(msum);
    const float* go = g_out ? g_out + ray * sumC : nullptr;
    int co = 0;
    for (int f = 0; f < n_fields; ++f) {
      const int C = channels[f];
      const float* v = fields[f] + s * C;
      float* gv = g_fields[f] ? g_fields[f] + s * C : nullptr;
      if (modes[f] == 2) {
        const float g = go ? go[co] / ((float)n * (float)C) : 0.f;
        if (gv) for (long e = 0; e < n * C; ++e) gv[e] = g;
        co += 1;
        continue;
      }
      for (long i = 0; i < n; ++i)
        for (int c = 0; c < C; ++c) {
          const float g = go ? go[co + c] : 0.f;
          if (gv) gv[i * C + c] = g * w[i] * inv;
          if (modes[f] == 0) A[i] += g * v[i * C + c];
        }
      co += C;
    }
    float aw = 0.f;
    for (long i = 0; i < n; ++i) aw += A[i] * w[i];
    const float gm = g_mask ? g_mask[ray] : 0.f;
    float suffix = 0.f;  // sum_{j > i} gw_j w_j
    for (long i = n - 1; i >= 0; --i) {
      const float gw = A[i] * inv - aw * inv * inv + gm;
      const float gtau = gw * T[i] - suffix;
      suffix += gw * w[i];
      if (g_density) g_density[s + i] = gtau * deltas[s + i];
      if (g_deltas) g_deltas[s + i] = gtau * density[s + i];
    }
  }
}
