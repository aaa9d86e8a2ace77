// Stand-alone run of the footprint-weighted hash-encoding twin (hashaa_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_hashgrid.h), so a table entry gathered through an index past its level, a radius read past S or an output written past S is an
// error report and a non-zero exit.  Sizes 0, 1 and 65; radius all 0, all +inf, all NaN and mixed (0, negative, NaN, +inf, tiny, huge, log-spaced);
// x exactly 0 and 1, outside the box and NaN; w_min 0 and 1/256; every F the contract allows; null optional arguments.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hashaa_host.cpp"

static int fail(const char* what, int F, int S) {
  fprintf(stderr, "hashaa_host_main: %s (F = %d, S = %d)\n", what, F, S);
  return 1;
}

static float lcg(uint32_t* s) {
  *s = *s * 1664525u + 1013904223u;
  return (float)(*s >> 8) / 16777216.f;
}

int main() {
  if (level_weight(0.f, 16, 0.f) != 1.f || level_weight(-1.f, 16, 0.5f) != 1.f || level_weight(NAN, 16, 0.5f) != 1.f) return fail("weight of a point sample", 0, 0);
  if (level_weight(INFINITY, 16, 0.f) != 0.f || level_weight(1e30f, 2048, 0.f) > 1e-30f) return fail("weight of an infinite footprint", 0, 0);
  if (level_weight(1e-30f, 16, 0.f) != 1.f || level_weight(1e-44f, 1, 0.f) != 1.f) return fail("weight of a tiny footprint", 0, 0);
  const int Fs[] = {1, 2, 4, 8}, Ss[] = {0, 1, 65};
  for (int F : Fs) {
    const int L = 32 / F, log2_T = 10;
    const long T = 1L << log2_T;
    uint32_t seed = 777u + (uint32_t)F;
    std::vector<int32_t> res(L);
    for (int l = 0; l < L; ++l) res[l] = 2 + 3 * l;  // dense up to res 9 ((res + 1)^3 <= 1024), hashed above
    std::vector<float> table((size_t)L * T * F);
    for (auto& v : table) v = 0.2f * lcg(&seed) - 0.1f;
    for (int S : Ss) {
      std::vector<float> x(3 * (size_t)S), g((size_t)S * L * F);
      for (auto& v : x) v = lcg(&seed);
      for (auto& v : g) v = 2.f * lcg(&seed) - 1.f;
      const float special[] = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 1.5f, 0.5f, 0.5f, NAN, 0.5f, 0.5f, 0.5f, -0.25f, INFINITY};
      for (int i = 0; i < 15 && i < 3 * S; ++i) x[i] = special[i];
      const float some[] = {0.f, -1.f, NAN, INFINITY, 1e-30f, 1e30f};
      for (int pattern = 0; pattern < 4; ++pattern) {
        std::vector<float> radius((size_t)S);
        for (int s = 0; s < S; ++s)
          radius[s] = pattern == 0 ? 0.f : pattern == 1 ? INFINITY : pattern == 2 ? NAN : (s % 11 < 6 ? some[s % 11] : expf(logf(1e-5f) + lcg(&seed) * logf(1e6f)));
        for (float w_min : {0.f, 1.f / 256.f}) {
          for (int inside_only = 0; inside_only < 2; ++inside_only) {
            std::vector<float> out((size_t)S * L * F), plain((size_t)S * L * F);
            if (hashaa_host_forward(x.data(), radius.data(), table.data(), res.data(), S, L, log2_T, F, w_min, inside_only, out.data())) return fail("forward refused", F, S);
            std::vector<float> zero((size_t)S, 0.f);
            hashaa_host_forward(x.data(), zero.data(), table.data(), res.data(), S, L, log2_T, F, w_min, inside_only, plain.data());
            for (int s = 0; s < S; ++s)
              for (int l = 0; l < L; ++l)
                for (int k = 0; k < F; ++k) {
                  const float o = out[((size_t)s * L + l) * F + k], p = plain[((size_t)s * L + l) * F + k];
                  if (!(fabsf(o) <= fabsf(p))) return fail("a weighted entry is not finite or exceeds the unweighted one", F, S);
                  if (pattern == 1 && o != 0.f) return fail("radius = inf must encode to zero", F, S);
                  if ((pattern == 0 || pattern == 2) && o != p) return fail("radius = 0 / NaN must encode like a point", F, S);
                }
          }
          std::vector<float> gT(table.size(), 0.f), gx(3 * (size_t)S, 7.f);
          if (hashaa_host_backward(x.data(), radius.data(), table.data(), res.data(), g.data(), S, L, log2_T, F, w_min, gT.data(), gx.data())) return fail("backward refused", F, S);
          for (auto v : gT) {
            if (!(fabsf(v) < 1e9f)) return fail("non-finite table gradient", F, S);
            if (pattern == 1 && v != 0.f) return fail("radius = inf must give a zero table gradient", F, S);
          }
          for (int s = 0; s < S; ++s)
            if (pattern == 1 && (gx[3 * s] != 0.f || gx[3 * s + 1] != 0.f || gx[3 * s + 2] != 0.f)) return fail("radius = inf must give a zero point gradient", F, S);
          // each gradient alone (the other pointer null)
          hashaa_host_backward(x.data(), radius.data(), table.data(), res.data(), g.data(), S, L, log2_T, F, w_min, nullptr, gx.data());
          hashaa_host_backward(x.data(), radius.data(), table.data(), res.data(), g.data(), S, L, log2_T, F, w_min, gT.data(), nullptr);
        }
      }
      std::vector<float> out((size_t)S * L * F), radius((size_t)S, 0.01f);
      if (hashaa_host_forward(x.data(), radius.data(), table.data(), res.data(), S, L, log2_T, F, 1.5f, 0, out.data()) != -1) return fail("w_min = 1.5 accepted", F, S);
      if (hashaa_host_forward(x.data(), radius.data(), table.data(), res.data(), S, L, log2_T, F, NAN, 0, out.data()) != -1) return fail("w_min = NaN accepted", F, S);
    }
  }
  printf("hashaa_host_main: ok\n");
  return 0;
}
