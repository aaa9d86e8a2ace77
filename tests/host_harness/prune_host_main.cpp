// Stand-alone run of the prune twin (prune/prune_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_prune.h), so a row written past the capacity, or a read past a ray's rows or past the list, is an error report and a
// non-zero exit.  It covers the truncation cases (cap = total, total - 1, 0), rays without rows, gaps of rows that no ray owns, a
// (start, count) that leaves [0, P) at either end, and R = 0 / P = 0; the values are checked elsewhere.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "prune/prune_host.cpp"

static int fail(const char* what) {
  fprintf(stderr, "prune_host_main: %s\n", what);
  return 1;
}

int main() {
  const int lengths[] = {0, 1, 2, 63, 64, 65, 129, 200, 0, 70};
  const long R = sizeof(lengths) / sizeof(lengths[0]) + 2;
  const float aabb[6] = {-0.12f, -0.10f, -0.15f, 0.12f, 0.14f, 0.09f};
  std::vector<int32_t> start(R), count(R);
  long P = 0;
  for (long r = 0; r < R - 2; ++r) {
    P += r % 3 == 1 ? 2 : 0;  // a gap in front of some rays
    start[r] = (int32_t)P;
    count[r] = lengths[r];
    P += lengths[r];
  }
  P += 5;  // five rows behind the last ray ...
  start[R - 2] = (int32_t)(P - 5), count[R - 2] = 65;  // ... owned by a ray whose count leaves the list: cut to 5
  start[R - 1] = -3, count[R - 1] = 10;                // a start in front of the list: no rows
  unsigned seed = 4711u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f; };
  std::vector<float> density(P), deltas(P), t(P), xyz(3 * P), dirs(3 * P);
  for (long i = 0; i < P; ++i) {
    density[i] = 200.f * rnd();
    deltas[i] = 1.f / 64.f;
    t[i] = rnd();
    for (int a = 0; a < 3; ++a) xyz[3 * i + a] = rnd(), dirs[3 * i + a] = rnd();
  }
  density[3] = NAN, density[4] = -1.f, density[5] = INFINITY;
  const float stops[3] = {9.2103404f, 0.f, INFINITY}, mins[3] = {0.f, 0.05f, 0.f};
  for (int c = 0; c < 3; ++c) {
    std::vector<uint8_t> keep(P, 0);
    std::vector<int32_t> new_count(R), new_start(R);
    prune_host_count(density.data(), deltas.data(), start.data(), count.data(), R, P, stops[c], mins[c], keep.data(), new_count.data());
    long total = 0;
    for (long r = 0; r < R; ++r) {
      new_start[r] = (int32_t)total;
      total += new_count[r];
    }
    if (new_count[0] || new_count[R - 1] || new_count[R - 2] > 5) return fail("unexpected counts");
    if (c == 2 && total != P - 2 * 3) return fail("both rules off must keep every owned row");  // (three gaps of two rows)
    if (c != 2 && (total < 2 || total >= P)) return fail("nothing pruned");
    const long caps[3] = {total, total - 1, 0};
    for (long cap : caps) {
      std::vector<float> t_o(cap), deltas_o(cap), xyz_o(3 * cap), dirs_o(3 * cap);
      std::vector<int32_t> ray_idx(cap), src_row(cap), count_out(R);
      int32_t tot = -1;
      uint8_t ovf = 2;
      prune_host_write(keep.data(), start.data(), count.data(), new_start.data(), R, P, cap, aabb, t.data(), deltas.data(), xyz.data(), dirs.data(),
                       t_o.data(), deltas_o.data(), xyz_o.data(), dirs_o.data(), ray_idx.data(), src_row.data(), count_out.data(), &tot, &ovf);
      long emitted = 0;
      for (long r = 0; r < R; ++r) emitted += count_out[r];
      if (tot != total || ovf != (total > cap) || emitted != (cap < total ? cap : total)) return fail("truncation");
      for (long i = 0; i < emitted; ++i)
        if (src_row[i] < 0 || src_row[i] >= P || !keep[src_row[i]] || t_o[i] != t[src_row[i]]) return fail("a survivor is not a copy of a kept row");
    }
  }
  // no rays, and no rows (null data pointers: nothing may be touched)
  int32_t tot = -1;
  uint8_t ovf = 2;
  std::vector<float> t_o(2), deltas_o(2), xyz_o(6), dirs_o(6);
  std::vector<int32_t> ray_idx(2), src_row(2);
  prune_host_count(nullptr, nullptr, nullptr, nullptr, 0, 0, 1.f, 0.f, nullptr, nullptr);
  prune_host_write(nullptr, nullptr, nullptr, nullptr, 0, 0, 2, aabb, nullptr, nullptr, nullptr, nullptr, t_o.data(), deltas_o.data(), xyz_o.data(),
                   dirs_o.data(), ray_idx.data(), src_row.data(), nullptr, &tot, &ovf);
  if (tot != 0 || ovf != 0 || ray_idx[1] != -1 || src_row[0] != -1) return fail("R = 0");
  std::vector<int32_t> s2 = {0, 4}, c2 = {3, 1}, n2(2), ns2 = {0, 0}, co2(2);
  prune_host_count(nullptr, nullptr, s2.data(), c2.data(), 2, 0, 1.f, 0.f, nullptr, n2.data());
  prune_host_write(nullptr, s2.data(), c2.data(), ns2.data(), 2, 0, 2, aabb, nullptr, nullptr, nullptr, nullptr, t_o.data(), deltas_o.data(), xyz_o.data(),
                   dirs_o.data(), ray_idx.data(), src_row.data(), co2.data(), &tot, &ovf);
  if (n2[0] || n2[1] || tot != 0 || ovf != 0 || co2[0] || co2[1]) return fail("P = 0");
  printf("prune_host_main: ok, %ld rows\n", P);
  return 0;
}
