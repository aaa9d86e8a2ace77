// Stand-alone run of the distortion twin (distort/distort_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_distort.h), so a read past a ray's rows or past the list, or a gradient written outside them, is an error report and a
// non-zero exit.  It covers rays without rows, the chunk edges (63 / 64 / 65 / 129 / 200 rows), gaps of rows that no ray owns, a
// (start, count) that leaves [0, P) at either end, each gradient asked for alone, and R = 0 / P = 0; the values are checked elsewhere.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "distort/distort_host.cpp"

static int fail(const char* what) {
  fprintf(stderr, "distort_host_main: %s\n", what);
  return 1;
}

int main() {
  const int lengths[] = {0, 1, 2, 63, 64, 65, 129, 200, 0, 70};
  const long R = sizeof(lengths) / sizeof(lengths[0]) + 2;
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
  std::vector<float> density(P), deltas(P), mid(P), width(P), g_loss(R);
  for (long i = 0; i < P; ++i) {
    density[i] = 8.f * rnd();
    deltas[i] = width[i] = 0.01f + 0.02f * rnd();
    mid[i] = 3.f + 0.03f * (float)i;  // (ascending along the list, so within every ray)
  }
  for (long r = 0; r < R; ++r) g_loss[r] = rnd() - 0.5f;
  const float sentinel = -7.f;
  std::vector<float> loss(R, sentinel);
  distort_host_forward(density.data(), deltas.data(), mid.data(), width.data(), start.data(), count.data(), R, P, loss.data());
  for (long r = 0; r < R; ++r) {
    const bool empty = r == R - 1 || count[r] == 0;
    if (!(loss[r] >= 0.f) || (empty && loss[r] != 0.f) || (!empty && loss[r] == 0.f)) return fail("loss");
  }
  for (int c = 0; c < 3; ++c) {  // both gradients, g_density alone, g_deltas alone
    std::vector<float> gd(P, sentinel), gl(P, sentinel);
    distort_host_backward(density.data(), deltas.data(), mid.data(), width.data(), start.data(), count.data(), R, P, g_loss.data(), c == 2 ? nullptr : gd.data(),
                          c == 1 ? nullptr : gl.data());
    long untouched = 0;
    for (long i = 0; i < P; ++i) {
      if (c != 2 && !isfinite(gd[i])) return fail("g_density");
      if (c != 1 && !isfinite(gl[i])) return fail("g_deltas");
      untouched += (c != 2 ? gd[i] : gl[i]) == sentinel;
    }
    if (untouched != 2 * 3) return fail("the rows of no ray were written");  // (three gaps of two rows)
  }
  distort_host_backward(density.data(), deltas.data(), mid.data(), width.data(), start.data(), count.data(), R, P, g_loss.data(), nullptr, nullptr);
  // no rays, and no rows (null data pointers: nothing may be touched)
  distort_host_forward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr);
  distort_host_backward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr);
  std::vector<int32_t> s2 = {0, 4}, c2 = {3, 1};
  std::vector<float> l2(2, sentinel), g2(2, 1.f), none(1, sentinel);
  distort_host_forward(nullptr, nullptr, nullptr, nullptr, s2.data(), c2.data(), 2, 0, l2.data());
  distort_host_backward(nullptr, nullptr, nullptr, nullptr, s2.data(), c2.data(), 2, 0, g2.data(), none.data(), none.data());
  if (l2[0] != 0.f || l2[1] != 0.f || none[0] != sentinel) return fail("P = 0");
  printf("distort_host_main: ok, %ld rows\n", P);
  return 0;
}
