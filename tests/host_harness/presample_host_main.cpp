// Stand-alone run of the resampling twin (presample/presample_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_presample.h), so a row written past the capacity, or a read past a ray's rows, past the list or past u, is an error report
// and a non-zero exit.  It feeds what breaks the preconditions -- unsorted u with values outside [0, 1] and NaN, weights that are NaN,
// negative or infinite, a (start, count) that leaves [0, P) at either end -- at the capacities total, total - 1 and 0, with eps = 0 and
// eps > 0, and R = 0 / P = 0; it checks that every written row lies inside its ray's rows, names a source row of that ray and that t never
// decreases within a ray.  The values themselves are checked elsewhere.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "presample/presample_host.cpp"

static int fail(const char* what) {
  fprintf(stderr, "presample_host_main: %s\n", what);
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
  std::vector<float> density(P), weights(P), deltas(P), t(P), origin(3 * R), dir(3 * R);
  for (long i = 0; i < P; ++i) {
    density[i] = 200.f * rnd();
    deltas[i] = 1.f / 64.f;
    t[i] = rnd();  // (unsorted on purpose)
  }
  for (long i = 0; i < 3 * R; ++i) origin[i] = rnd() - 0.5f, dir[i] = rnd() - 0.5f;
  dir[3] = dir[4] = dir[5] = 0.f;  // ray 1: |dir| = 0
  density[3] = NAN, density[4] = -1.f, density[5] = INFINITY;
  std::vector<float> trans(R);
  presample_host_weights(density.data(), deltas.data(), start.data(), count.data(), R, P, weights.data(), trans.data());
  presample_host_weights(density.data(), deltas.data(), start.data(), count.data(), R, P, weights.data(), nullptr);
  if (trans[0] != 1.f || trans[R - 1] != 1.f) return fail("a ray without rows must be transparent");
  for (long i = 0; i < P; i += 7) weights[i] = NAN;
  for (long i = 3; i < P; i += 11) weights[i] = -1.f;
  for (long i = 5; i < P; i += 13) weights[i] = 0.f;
  weights[P - 2] = INFINITY;
  const int n_imps[3] = {1, 65, 130};
  const float epss[2] = {0.f, 1e-5f};
  for (int n_imp : n_imps)
    for (float eps : epss)
      for (int with_u = 0; with_u < 2; ++with_u) {
        std::vector<float> u(R * n_imp), cdf(P, -7.5f), mass(R);
        for (float& x : u) x = 1.5f * rnd() - 0.25f;  // unsorted, some outside [0, 1]
        u[0] = NAN;
        std::vector<int32_t> new_count(R), new_start(R);
        presample_host_count(weights.data(), start.data(), count.data(), R, P, n_imp, eps, cdf.data(), mass.data(), new_count.data());
        long total = 0;
        for (long r = 0; r < R; ++r) {
          new_start[r] = (int32_t)total;
          total += new_count[r];
          if (new_count[r] != 0 && new_count[r] != n_imp) return fail("a count is neither 0 nor n_imp");
        }
        // (ray 3 starts at the infinite density of row 5, whose weight was then set to 0: it has no mass unless eps gives it some)
        if (new_count[0] || new_count[R - 1] || !new_count[R - 2] || !new_count[4] || (new_count[3] != 0) != (eps > 0.f)) return fail("unexpected counts");
        const long caps[3] = {total, total - 1, 0};
        for (long cap : caps) {
          std::vector<float> t_o(cap), deltas_o(cap), xyz_o(3 * cap), dirs_o(3 * cap);
          std::vector<int32_t> ray_idx(cap), src_row(cap), count_out(R);
          int32_t tot = -1;
          uint8_t ovf = 2;
          presample_host_write(weights.data(), cdf.data(), mass.data(), t.data(), deltas.data(), start.data(), count.data(), new_start.data(), R, P, origin.data(),
                               dir.data(), with_u ? u.data() : nullptr, n_imp, eps, cap, aabb, t_o.data(), deltas_o.data(), xyz_o.data(), dirs_o.data(),
                               ray_idx.data(), src_row.data(), count_out.data(), &tot, &ovf);
          long emitted = 0;
          for (long r = 0; r < R; ++r) {
            const lab4d_prune::Rows rr = lab4d_prune::rows_of(start.data(), count.data(), r, P);
            for (long i = new_start[r]; i < new_start[r] + count_out[r]; ++i) {
              if (ray_idx[i] != r || src_row[i] < rr.s || src_row[i] >= rr.s + rr.n) return fail("a row outside its ray");
              if (i > new_start[r] && !(t_o[i] >= t_o[i - 1])) return fail("t decreases within a ray");
              if (!(deltas_o[i] <= deltas[src_row[i]])) return fail("a span longer than its source row");
            }
            emitted += count_out[r];
          }
          if (tot != total || ovf != (total > cap) || emitted != (cap < total ? cap : total)) return fail("truncation");
        }
      }
  // no rays, and no rows (null data pointers: nothing may be touched)
  int32_t tot = -1;
  uint8_t ovf = 2;
  std::vector<float> t_o(2), deltas_o(2), xyz_o(6), dirs_o(6);
  std::vector<int32_t> ray_idx(2), src_row(2);
  presample_host_weights(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr);
  presample_host_count(nullptr, nullptr, nullptr, 0, 0, 4, 1e-5f, nullptr, nullptr, nullptr);
  presample_host_write(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 4, 1e-5f, 2, aabb, t_o.data(),
                       deltas_o.data(), xyz_o.data(), dirs_o.data(), ray_idx.data(), src_row.data(), nullptr, &tot, &ovf);
  if (tot != 0 || ovf != 0 || ray_idx[1] != -1 || src_row[0] != -1) return fail("R = 0");
  std::vector<int32_t> s2 = {0, 4}, c2 = {3, 1}, n2(2), ns2 = {0, 0}, co2(2);
  std::vector<float> m2(2), o2(6, 0.f), d2(6, 1.f);
  presample_host_count(nullptr, s2.data(), c2.data(), 2, 0, 4, 1e-5f, nullptr, m2.data(), n2.data());
  presample_host_write(nullptr, nullptr, m2.data(), nullptr, nullptr, s2.data(), c2.data(), ns2.data(), 2, 0, o2.data(), d2.data(), nullptr, 4, 1e-5f, 2, aabb,
                       t_o.data(), deltas_o.data(), xyz_o.data(), dirs_o.data(), ray_idx.data(), src_row.data(), co2.data(), &tot, &ovf);
  if (n2[0] || n2[1] || m2[0] != 0.f || tot != 0 || ovf != 0 || co2[0] || co2[1]) return fail("P = 0");
  printf("presample_host_main: ok, %ld rows\n", P);
  return 0;
}
