// Stand-alone run of the hash-SDF twin (hashsdf_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_hashsdf.h), so a table entry gathered through an index past its level, or an output written past S, is an error report
// and a non-zero exit.  It covers the special points of the rules: x01 exactly 0 and exactly 1, a point outside the box, a NaN point, 64
// identical points, 130 consecutive samples of a ray; every F the contract allows; null optional arguments.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hashsdf_host.cpp"

static int fail(const char* what, int F) {
  fprintf(stderr, "hashsdf_host_main: %s (F = %d)\n", what, F);
  return 1;
}

static float lcg(uint32_t* s) {
  *s = *s * 1664525u + 1013904223u;
  return (float)(*s >> 8) / 16777216.f * 2.f - 1.f;
}

int main() {
  const int Fs[] = {1, 2, 4, 8};
  for (int F : Fs) {
    const int L = 32 / F, log2_T = 10;
    const long T = 1L << log2_T;
    uint32_t seed = 12345u + (uint32_t)F;
    std::vector<int32_t> res(L);
    for (int l = 0; l < L; ++l) res[l] = 2 + 3 * l;  // dense up to res 9 ((res + 1)^3 <= 1024), hashed above
    std::vector<float> table((size_t)L * T * F), W1(64 * 32), b1(64), w2(64), b2(1);
    for (auto& v : table) v = 0.1f * lcg(&seed);
    for (auto& v : W1) v = 0.2f * lcg(&seed);
    for (auto& v : b1) v = 0.2f * lcg(&seed);
    for (auto& v : w2) v = 0.2f * lcg(&seed);
    b2[0] = 0.05f;
    std::vector<float> x = {0.f, 0.f, 0.f, 1.f, 1.f, 1.f, 0.f, 0.5f, 1.f, 1.5f, 0.5f, 0.5f, -0.25f, 0.5f, 0.5f, NAN, 0.5f, 0.5f, 0.5f, INFINITY, 0.5f};
    const long first_same = (long)x.size() / 3;
    for (int i = 0; i < 64; ++i) x.insert(x.end(), {0.3f, 0.6f, 0.2f});
    for (int i = 0; i < 130; ++i) {
      const float t = (i + 0.5f) / 130.f;
      x.insert(x.end(), {0.05f + 0.9f * t, 0.1f + 0.7f * t, 0.9f - 0.8f * t});
    }
    const long S = (long)x.size() / 3;
    std::vector<float> sdf(S), grad(3 * S), gs(S), gg(3 * S);
    for (auto& v : gs) v = lcg(&seed);
    for (auto& v : gg) v = lcg(&seed);
    if (hashsdf_host_forward(x.data(), table.data(), res.data(), S, L, log2_T, F, W1.data(), b1.data(), w2.data(), b2.data(), sdf.data(), grad.data()))
      return fail("forward refused", F);
    float outside = b2[0];
    for (int j = 0; j < 64; ++j) outside += b1[j] > 0.f ? w2[j] * b1[j] : 0.f;
    for (long s = 3; s < 7; ++s) {
      if (fabsf(sdf[s] - outside) > 1e-6f) return fail("sdf outside the box", F);
      if (grad[3 * s] != 0.f || grad[3 * s + 1] != 0.f || grad[3 * s + 2] != 0.f) return fail("grad01 outside the box", F);
    }
    for (long s = 0; s < S; ++s)
      if (!(fabsf(sdf[s]) < 1e6f) || !(fabsf(grad[3 * s]) < 1e6f)) return fail("non-finite output", F);
    for (long s = first_same + 1; s < first_same + 64; ++s)
      if (sdf[s] != sdf[first_same] || grad[3 * s + 1] != grad[3 * first_same + 1]) return fail("identical points differ", F);
    // sdf alone (null grad01), then the adjoint: everything, and every null pattern of the contract
    std::vector<float> sdf2(S);
    hashsdf_host_forward(x.data(), table.data(), res.data(), S, L, log2_T, F, W1.data(), b1.data(), w2.data(), b2.data(), sdf2.data(), nullptr);
    for (long s = 0; s < S; ++s)
      if (sdf2[s] != sdf[s]) return fail("sdf with a null grad01", F);
    std::vector<float> gT(table.size(), 0.f), gW1(64 * 32), gb1(64), gw2(64), gb2(1), gT2(table.size(), 0.f), gW1b(64 * 32);
    const int rows[] = {1, 3, 512};
    for (int n : rows) {
      std::fill(gT.begin(), gT.end(), 0.f);
      if (hashsdf_host_backward(x.data(), table.data(), res.data(), S, L, log2_T, F, W1.data(), b1.data(), w2.data(), gs.data(), gg.data(), gT.data(), gW1.data(),
                                gb1.data(), gw2.data(), gb2.data(), n))
        return fail("backward refused", F);
      float sum = 0.f;
      for (long s = 0; s < S; ++s) sum += gs[s];
      if (fabsf(gb2[0] - sum) > 1e-3f) return fail("db2 is not the sum of gs", F);
      for (auto v : gT)
        if (!(fabsf(v) < 1e9f)) return fail("non-finite table gradient", F);
    }
    hashsdf_host_backward(x.data(), table.data(), res.data(), S, L, log2_T, F, W1.data(), b1.data(), w2.data(), gs.data(), nullptr, gT2.data(), nullptr, nullptr,
                          nullptr, nullptr, 3);
    hashsdf_host_backward(x.data(), table.data(), res.data(), S, L, log2_T, F, W1.data(), b1.data(), w2.data(), nullptr, gg.data(), nullptr, gW1b.data(), nullptr,
                          nullptr, nullptr, 3);
    // the points outside the box alone: no table gradient, no dW1
    std::fill(gT2.begin(), gT2.end(), 0.f);
    hashsdf_host_backward(x.data() + 9, table.data(), res.data(), 4, L, log2_T, F, W1.data(), b1.data(), w2.data(), gs.data(), gg.data(), gT2.data(), gW1b.data(),
                          gb1.data(), gw2.data(), gb2.data(), 2);
    for (auto v : gT2)
      if (v != 0.f) return fail("table gradient from outside the box", F);
    for (auto v : gW1b)
      if (v != 0.f) return fail("dW1 from outside the box", F);
    // no samples
    hashsdf_host_backward(nullptr, table.data(), res.data(), 0, L, log2_T, F, W1.data(), b1.data(), w2.data(), gs.data(), gg.data(), gT2.data(), gW1b.data(),
                          gb1.data(), gw2.data(), gb2.data(), 2);
    if (gb2[0] != 0.f || gW1b[5] != 0.f) return fail("S = 0 must write zero dense gradients", F);
    if (hashsdf_host_forward(x.data(), table.data(), res.data(), S, L + 1, log2_T, F, W1.data(), b1.data(), w2.data(), b2.data(), sdf.data(), nullptr) != -1)
      return fail("L * F != 32 accepted", F);
  }
  printf("hashsdf_host_main: ok\n");
  return 0;
}
