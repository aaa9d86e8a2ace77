// Stand-alone run of the sphere-tracing twin (hashtrace/hashtrace_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_hashtrace.h), so a table read past a level's slab or an output written past the rays is an error report and a non-zero exit.
// The field is the analytic one of tests/hashtrace_checks.py (a sphere's distance at the vertices of the first level, W1 rows 0 / 1 = +-e_0);
// the rays are the degenerate ones of the rules: axis-parallel, d = 0, NaN or inf in each input, t0 > t1, t0 == t1, a ray grazing a box edge,
// a box miss, rays that start inside, and R = 0.  The statuses are checked here, the values elsewhere.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hashtrace/hashtrace_host.cpp"

static int fail(const char* what, long r) {
  fprintf(stderr, "hashtrace_host_main: %s (ray %ld)\n", what, r);
  return 1;
}

int main() {
  const int L = 16, F = 2, log2_T = 12, n_min = 8, n_max = 64;
  const float aabb[6] = {-0.12f, -0.12f, -0.12f, 0.12f, 0.12f, 0.12f}, radius = 0.08f;
  std::vector<int32_t> res(L);
  for (int l = 0; l < L; ++l) res[l] = (int32_t)floor(n_min * exp(l * (log((double)n_max) - log((double)n_min)) / (L - 1)) + 1e-9);
  std::vector<float> table((size_t)L << log2_T << 1, 0.f), W1(64 * 32, 0.f), b1(64, 0.f), w2(64, 0.f), b2(1, 0.f);
  const int n = res[0] + 1;  // level 0 is dense: (8 + 1)^3 <= 2^12
  for (int iz = 0; iz < n; ++iz)
    for (int iy = 0; iy < n; ++iy)
      for (int ix = 0; ix < n; ++ix) {
        const double x = aabb[0] + 0.24 * ix / res[0], y = aabb[1] + 0.24 * iy / res[0], z = aabb[2] + 0.24 * iz / res[0];
        table[(size_t)(ix + n * (iy + n * iz)) * F] = (float)(sqrt(x * x + y * y + z * z) - radius);
      }
  W1[0] = 1.f, W1[32] = -1.f, w2[0] = 1.f, w2[1] = -1.f;

  struct Ray { float o[3], d[3], t0, t1; int want; };  // want: the status at max_steps = 128; -1 = a hit (1 or 2); -2 = status 0 without an evaluation, at every setting
  const float nan = NAN, inf = INFINITY;
  const std::vector<Ray> rays = {
      {{0.f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 0.f, 2.f, -1},              // axis-parallel, through the centre
      {{0.01f, -0.5f, 0.02f}, {0.f, 2.f, 0.f}, 0.f, 2.f, -1},          // axis-parallel, |d| = 2
      {{0.f, 0.f, -0.5f}, {0.f, 0.f, 0.f}, 0.f, 2.f, -2},               // d = 0
      {{nan, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 0.f, 2.f, -2},               // NaN / inf in each input
      {{0.f, 0.f, -0.5f}, {0.f, inf, 1.f}, 0.f, 2.f, -2},
      {{0.f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, nan, 2.f, -2},
      {{0.f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 0.f, inf, -2},
      {{0.f, -inf, -0.5f}, {0.f, 0.f, 1.f}, 0.f, 2.f, -2},
      {{0.f, 0.f, -0.5f}, {nan, 0.f, 1.f}, 0.f, 2.f, -2},
      {{0.f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 2.f, 1.f, -2},               // t0 > t1
      {{0.f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 0.45f, 0.45f, 3},           // t0 == t1, inside the sphere
      {{0.f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 0.39f, 0.39f, 0},           // t0 == t1, in the box, outside the sphere: MISS at t_exit = t0
      {{0.f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 0.1f, 0.1f, -2},             // t0 == t1 in front of the box
      {{0.12f, 0.12f, -0.5f}, {0.f, 0.f, 1.f}, 0.f, 2.f, 0},           // along a box edge
      {{-0.5f, 0.74f, 0.f}, {1.f, -1.f, 0.f}, 0.f, 2.f, 0},            // touches the box edge x = hi, y = hi in one point
      {{0.3f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 0.f, 2.f, -2},              // a box miss, parallel axis outside
      {{0.f, 0.f, -0.5f}, {0.3f, 0.3f, -1.f}, 0.f, 2.f, -2},            // a box miss, pointing away
      {{0.01f, 0.02f, 0.f}, {1.f, 0.f, 0.f}, 0.f, 2.f, 3},             // starts inside the sphere
      {{0.1f, 0.f, -0.5f}, {0.f, 0.f, 1.f}, 0.f, 2.f, 0},              // through the box beside the sphere
  };
  const long R = (long)rays.size();
  std::vector<float> origin(3 * R), dir(3 * R), t_range(2 * R), t_hit(R), sdf_hit(R);
  std::vector<int32_t> status(R), n_eval(R);
  for (long r = 0; r < R; ++r) {
    for (int a = 0; a < 3; ++a) origin[3 * r + a] = rays[r].o[a], dir[3 * r + a] = rays[r].d[a];
    t_range[2 * r] = rays[r].t0, t_range[2 * r + 1] = rays[r].t1;
  }
  const int settings[3][2] = {{128, 8}, {1, 0}, {7, 32}};  // max_steps, n_bisect
  for (const auto& st : settings) {
    for (long r = 0; r < R; ++r) t_hit[r] = sdf_hit[r] = 7.f, status[r] = n_eval[r] = -7;
    if (hashtrace_host_trace(origin.data(), dir.data(), t_range.data(), aabb, R, table.data(), res.data(), L, log2_T, F, W1.data(), b1.data(), w2.data(),
                             b2.data(), 1e-4f, 1.f, 1e-4f, st[0], st[1], t_hit.data(), status.data(), n_eval.data(), sdf_hit.data()))
      return fail("the twin refused good arguments", -1);
    for (long r = 0; r < R; ++r) {
      if (status[r] < 0 || status[r] > 4 || n_eval[r] < 0 || n_eval[r] > st[0] + st[1]) return fail("status or n_eval outside its range", r);
      if (rays[r].want == -2 ? (status[r] != 0 || n_eval[r] != 0) : (st[0] == 128 && (rays[r].want < 0 ? status[r] != 1 && status[r] != 2 : status[r] != rays[r].want)))
        return fail("unexpected status", r);
      if (n_eval[r] == 0 && (status[r] != 0 || sdf_hit[r] != 0.f || !(t_hit[r] == rays[r].t0 || (isnan(t_hit[r]) && isnan(rays[r].t0)))))
        return fail("a ray without an evaluation: status 0, t_hit = t0, sdf_hit = 0", r);
      if (n_eval[r] > 0 && !(t_hit[r] >= rays[r].t0 && t_hit[r] <= rays[r].t1)) return fail("t_hit outside [t0, t1]", r);
    }
  }
  // R = 0: nothing is read or written (NULL everywhere but the checked scalars)
  if (hashtrace_host_trace(nullptr, nullptr, nullptr, aabb, 0, table.data(), res.data(), L, log2_T, F, W1.data(), b1.data(), w2.data(), b2.data(), 1e-4f, 1.f,
                           1e-4f, 128, 8, nullptr, nullptr, nullptr, nullptr))
    return fail("R = 0 must succeed", -1);
  if (hashtrace_host_trace(origin.data(), dir.data(), t_range.data(), aabb, R, table.data(), res.data(), L, log2_T, F, W1.data(), b1.data(), w2.data(),
                           b2.data(), 0.f, 1.f, 1e-4f, 128, 8, t_hit.data(), status.data(), n_eval.data(), sdf_hit.data()) != -1)
    return fail("eps = 0 must be refused", -1);
  printf("hashtrace_host_main: ok, %ld rays\n", R);
  return 0;
}
