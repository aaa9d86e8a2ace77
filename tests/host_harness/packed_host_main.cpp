// Stand-alone run of the packed twin (packed_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_packed.h), so a row written past the capacity, or a read past a ray's rows, is an error report and a non-zero exit.  It
// covers the truncation cases (cap = total, total - 1, 0) and rays without samples, on a small grid; the values are checked elsewhere.
#include <stdio.h>
#include <stdlib.h>

#include "packed_host.cpp"

static int fail(const char* what) {
  fprintf(stderr, "packed_host_main: %s\n", what);
  return 1;
}

int main() {
  const int G = 5, k_max = 40;
  const long R = 37;
  const float dt = 0.03125f;
  const float aabb[6] = {-0.12f, -0.10f, -0.15f, 0.12f, 0.14f, 0.09f};
  std::vector<uint32_t> bits(occ::n_words(G), 0u);
  for (long i = 0; i < occ::n_cells(G); ++i)
    if (i % 3 != 1) bits[i >> 5] |= 1u << (i & 31);
  std::vector<float> origin(3 * R), dir(3 * R), t_range(2 * R);
  unsigned seed = 12345u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f; };
  for (long r = 0; r < R; ++r) {
    for (int a = 0; a < 3; ++a) {
      origin[3 * r + a] = aabb[a] - 0.2f + 0.1f * rnd();
      dir[3 * r + a] = 0.3f + 0.5f * rnd();
    }
    t_range[2 * r] = 0.f;
    t_range[2 * r + 1] = 1.5f;
  }
  dir[3 * 5] = dir[3 * 5 + 1] = 0.f;                   // axis-parallel
  origin[3 * 6] = NAN;                                // non-finite: nothing kept
  t_range[2 * 7] = 2.f, t_range[2 * 7 + 1] = 1.f;     // t0 > t1: nothing kept
  for (int a = 0; a < 3; ++a) dir[3 * 8 + a] = -1.f;  // pointing away: a miss
  std::vector<int32_t> count(R), start(R);
  packed_host_march_count(origin.data(), dir.data(), t_range.data(), aabb, bits.data(), G, R, dt, k_max, count.data());
  long total = 0;
  for (long r = 0; r < R; ++r) {
    start[r] = (int32_t)total;
    total += count[r];
  }
  if (total < 2 || count[6] || count[7] || count[8]) return fail("unexpected counts");
  const long caps[3] = {total, total - 1, 0};
  for (long cap : caps) {
    std::vector<float> t(cap), deltas(cap), xyz(3 * cap), dirs(3 * cap);
    std::vector<int32_t> ray_idx(cap), count_out(R);
    int32_t tot = -1;
    uint8_t ovf = 2;
    packed_host_march_write(origin.data(), dir.data(), t_range.data(), aabb, bits.data(), G, R, dt, k_max, start.data(), cap, t.data(), deltas.data(),
                            xyz.data(), dirs.data(), ray_idx.data(), count_out.data(), &tot, &ovf);
    long kept = 0;
    for (long r = 0; r < R; ++r) kept += count_out[r];
    if (tot != total || ovf != (total > cap) || kept != (cap < total ? cap : total)) return fail("truncation");
    // composite the truncated list: rays 6, 7, 8 (and, at cap = 0, all) have no samples
    std::vector<float> density(cap), rgb(3 * cap), mask(R), out(R * 5), w(cap), T(cap), g_out(R * 5, 1.f), g_mask(R, 1.f), g_density(cap), g_deltas(cap),
        g_rgb(3 * cap), g_t(cap);
    for (long i = 0; i < cap; ++i) {
      density[i] = 5.f * rnd();
      for (int a = 0; a < 3; ++a) rgb[3 * i + a] = rnd();
    }
    const float* fields[3] = {rgb.data(), t.data(), rgb.data()};
    float* g_fields[3] = {g_rgb.data(), g_t.data(), nullptr};
    const int channels[3] = {3, 1, 3}, modes[3] = {0, 1, 2};
    packed_host_composite_forward(density.data(), deltas.data(), 3, fields, channels, modes, start.data(), count_out.data(), R, cap, w.data(), T.data(),
                                  mask.data(), out.data());
    packed_host_composite_backward(density.data(), deltas.data(), 3, fields, channels, modes, start.data(), count_out.data(), R, cap, g_mask.data(),
                                   g_out.data(), g_density.data(), g_deltas.data(), g_fields);
    for (long r = 0; r < R; ++r) {
      if (!(mask[r] >= 0.f && mask[r] <= 1.0001f)) return fail("mask outside [0, 1]");
      if (count_out[r] == 0)
        for (int c = 0; c < 5; ++c)
          if (out[r * 5 + c] != 0.f || mask[r] != 0.f) return fail("a ray without samples must render zeros");
    }
  }
  printf("packed_host_main: ok, %ld samples\n", total);
  return 0;
}
