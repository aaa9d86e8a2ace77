// CPU build of the footprint-weighted hash encoding (lab4d_amd/csrc/hashgrid_math.hpp: level_weight over encode_level / encode_level_bwd), the
// serial twin of the AA kernels of csrc/hashgrid.hip (see hashgrid_host.cpp).  TEST INFRASTRUCTURE ONLY.
#include "hashgrid_math.hpp"

using namespace lab4d_hash;

static bool inside01(const float* p) { return p[0] >= 0.f && p[0] <= 1.f && p[1] >= 0.f && p[1] <= 1.f && p[2] >= 0.f && p[2] <= 1.f; }  // (NaN: outside)

extern "C" int hashaa_host_forward(const float* x, const float* radius, const float* table, const int* res, int S, int L, int log2_T, int F, float w_min,
                                   int inside_only, float* out) {
  if (S < 0 || L <= 0 || F < 1 || F > MAXF || !(w_min >= 0.f && w_min <= 1.f)) return -1;
  const size_t slab = ((size_t)1 << log2_T) * F;
  for (long s = 0; s < S; ++s) {
    float* row = out + (size_t)s * L * F;
    if (inside_only && !inside01(x + 3 * s)) {
      for (int k = 0; k < L * F; ++k) row[k] = 0.f;
      continue;
    }
    for (int l = 0; l < L; ++l) {
      const float w = level_weight(radius[s], res[l], w_min);
      if (w == 0.f) {  // nothing of the level is read
        for (int k = 0; k < F; ++k) row[l * F + k] = 0.f;
        continue;
      }
      float f[MAXF];
      encode_level(x + 3 * s, table + l * slab, res[l], log2_T, F, f);
      for (int k = 0; k < F; ++k) row[l * F + k] = f[k] * w;
    }
  }
  return 0;
}

// g_table (zero-filled by the caller, may be null) accumulated, g_x (may be null) written
extern "C" int hashaa_host_backward(const float* x, const float* radius, const float* table, const int* res, const float* g_out, int S, int L, int log2_T,
                                    int F, float w_min, float* g_table, float* g_x) {
  if (S < 0 || L <= 0 || F < 1 || F > MAXF || !(w_min >= 0.f && w_min <= 1.f)) return -1;
  const size_t slab = ((size_t)1 << log2_T) * F;
  for (long s = 0; s < S; ++s) {
    float gx[3] = {0.f, 0.f, 0.f};
    for (int l = 0; l < L; ++l) {
      const float w = level_weight(radius[s], res[l], w_min);
      float g[MAXF];
      for (int k = 0; k < F; ++k) g[k] = g_out[(size_t)s * L * F + l * F + k] * w;
      encode_level_bwd(x + 3 * s, table + l * slab, res[l], log2_T, F, g, g_table ? g_table + l * slab : nullptr, g_x ? gx : nullptr);
    }
    if (g_x) { g_x[3 * s] = gx[0]; g_x[3 * s + 1] = gx[1]; g_x[3 * s + 2] = gx[2]; }
  }
  return 0;
}

extern "C" float hashaa_host_level_weight(float radius, int res, float w_min) { return level_weight(radius, res, w_min); }
