// Stand-alone run of the cone-march twin (conemarch/conemarch_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_conemarch.h), so a row written past the capacity, or a word read past a level's bits, is an error report and a non-zero
// exit.  It covers K = 1 and K = 4, the truncation cases (cap = total, total - 1, a cut inside a ray, 0) and rays without samples, on a
// small grid; the values are checked elsewhere.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "conemarch/conemarch_host.cpp"

static int fail(const char* what) {
  fprintf(stderr, "conemarch_host_main: %s\n", what);
  return 1;
}

static int run(int K, long* samples) {
  const int G = 4, k_max = 48;
  const long R = 37;
  const float cone_angle = 0.05f, dt_min = 0.02f, dt_max = 0.5f;
  const float base[6] = {-0.12f, -0.10f, -0.15f, 0.12f, 0.14f, 0.09f};
  std::vector<float> aabbs(6 * K);
  for (int c = 0; c < K; ++c)
    for (int a = 0; a < 3; ++a) {
      const double mid = 0.5 * ((double)base[a] + base[3 + a]), half = 0.5 * ((double)base[3 + a] - base[a]) * (double)(1 << c);
      aabbs[6 * c + a] = (float)(mid - half);
      aabbs[6 * c + 3 + a] = (float)(mid + half);
    }
  const long W = occ::n_words(G);
  std::vector<uint32_t> bits(K * W, 0u);
  for (int c = 0; c < K; ++c)
    for (long i = 0; i < occ::n_cells(G); ++i)
      if ((i + c) % 3 != 1) bits[c * W + (i >> 5)] |= 1u << (i & 31);
  const float* outer = aabbs.data() + 6 * (K - 1);
  std::vector<float> origin(3 * R), dir(3 * R), t_range(2 * R);
  unsigned seed = 4321u + (unsigned)K;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f; };
  for (long r = 0; r < R; ++r) {
    for (int a = 0; a < 3; ++a) {
      const float ext = outer[3 + a] - outer[a];
      origin[3 * r + a] = outer[a] - 0.2f * ext + 0.1f * ext * rnd();
      dir[3 * r + a] = ext * (0.3f + 0.5f * rnd());
    }
    t_range[2 * r] = 0.f;
    t_range[2 * r + 1] = 3.f;
  }
  for (int a = 0; a < 3; ++a) origin[3 * 4 + a] = 0.5f * (base[a] + base[3 + a]);  // inside level 0
  dir[3 * 5] = dir[3 * 5 + 1] = 0.f;                                               // axis-parallel
  origin[3 * 6] = NAN;                                                             // non-finite: nothing kept
  t_range[2 * 7] = 2.f, t_range[2 * 7 + 1] = 1.f;                                  // t0 > t1: nothing kept
  for (int a = 0; a < 3; ++a) dir[3 * 8 + a] = -1.f;                               // pointing away: a miss
  t_range[2 * 9] = -1.f;                                                           // t0 < 0
  dir[3 * 10] = dir[3 * 10 + 1] = dir[3 * 10 + 2] = 0.f;                           // |d| = 0: rejected
  std::vector<int32_t> count(R), start(R);
  conemarch_host_count(origin.data(), dir.data(), t_range.data(), aabbs.data(), bits.data(), K, G, R, cone_angle, dt_min, dt_max, k_max, count.data());
  long total = 0, inside = -1;
  for (long r = 0; r < R; ++r) {
    start[r] = (int32_t)total;
    total += count[r];
    if (count[r] >= 2 && inside < 0) inside = start[r] + 1;  // a cut inside a ray
  }
  if (total < 2 || inside < 0 || count[6] || count[7] || count[8] || count[10]) return fail("unexpected counts");
  const long caps[4] = {total, total - 1, inside, 0};
  for (long cap : caps) {
    std::vector<float> t(cap), steps(cap), deltas(cap), xyz(3 * cap), dirs(3 * cap);
    std::vector<int32_t> ray_idx(cap), level(cap), count_out(R);
    int32_t tot = -1;
    uint8_t ovf = 2;
    conemarch_host_write(origin.data(), dir.data(), t_range.data(), aabbs.data(), bits.data(), K, G, R, cone_angle, dt_min, dt_max, k_max, start.data(), cap,
                         t.data(), steps.data(), deltas.data(), xyz.data(), dirs.data(), ray_idx.data(), level.data(), count_out.data(), &tot, &ovf);
    long kept = 0;
    for (long r = 0; r < R; ++r) kept += count_out[r];
    if (tot != total || ovf != (total > cap) || kept != (cap < total ? cap : total)) return fail("truncation");
    for (long i = 0; i < kept; ++i)
      if (level[i] < 0 || level[i] >= K || !(steps[i] >= dt_min && steps[i] <= dt_max)) return fail("a row's level or step");
    // the written points through the per-point call, with and without delta and level
    std::vector<uint8_t> mask(cap);
    std::vector<int32_t> lv(cap);
    conemarch_host_cascade_mask(xyz.data(), deltas.data(), aabbs.data(), bits.data(), K, G, cap, mask.data(), lv.data());
    for (long i = 0; i < kept; ++i)
      if (!mask[i] || lv[i] != level[i]) return fail("cascade_mask disagrees with the march");
    conemarch_host_cascade_mask(xyz.data(), nullptr, aabbs.data(), bits.data(), K, G, cap, mask.data(), nullptr);
  }
  *samples += total;
  return 0;
}

int main() {
  long samples = 0;
  if (run(1, &samples) || run(4, &samples)) return 1;
  printf("conemarch_host_main: ok, %ld samples\n", samples);
  return 0;
}
