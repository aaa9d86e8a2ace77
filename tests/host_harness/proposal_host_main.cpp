// Stand-alone run of the proposal-loss twin (proposal/proposal_host.cpp) for the sanitizers: tests/host_twin.py builds this file with
// g++ -fsanitize=address,undefined and runs it as a child process.  Every buffer is a heap block of exactly the size the contract names
// (include/lab4d_proposal.h), so a read past a ray's rows, past a list, or an index of the span outside the envelope's prefixes is an error
// report and a non-zero exit.  It feeds what breaks the preconditions -- weights that are NaN, negative or infinite in both lists, envelopes
// that are NOT monotone (random t, random and NaN t), a (start, count) that leaves [0, P) at either end, |dir| = 0 -- with eps = 0 and
// eps > 0, and R = 0 / Pe = 0 / Pf = 0; it checks that every span lies in [0, n_e], that the loss is >= 0 or NaN-free where the input is,
// and that the adjoint is 0 where w_e is not > 0.  The values themselves are checked elsewhere.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "proposal/proposal_host.cpp"

static int fail(const char* what) {
  fprintf(stderr, "proposal_host_main: %s\n", what);
  return 1;
}

struct List {
  std::vector<int32_t> start, count;
  std::vector<float> w, t, deltas;
  long P = 0;
};

int main() {
  const int len_e[] = {0, 1, 2, 63, 64, 65, 129, 200, 0, 70, 5, 64};
  const int len_f[] = {3, 0, 65, 64, 1, 200, 63, 129, 0, 2, 130, 65};
  const long R = sizeof(len_e) / sizeof(len_e[0]) + 2;
  unsigned seed = 4711u;
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) / 16777216.f; };
  auto make = [&](const int* lengths, bool sorted) {
    List l;
    l.start.resize(R), l.count.resize(R);
    for (long r = 0; r < R - 2; ++r) {
      l.P += r % 3 == 1 ? 2 : 0;  // a gap in front of some rays
      l.start[r] = (int32_t)l.P;
      l.count[r] = lengths[r];
      l.P += lengths[r];
    }
    l.P += 5;                                                    // five rows behind the last ray ...
    l.start[R - 2] = (int32_t)(l.P - 5), l.count[R - 2] = 65;    // ... owned by a ray whose count leaves the list: cut to 5
    l.start[R - 1] = -3, l.count[R - 1] = 10;                    // a start in front of the list: no rows
    l.w.resize(l.P), l.t.resize(l.P), l.deltas.resize(l.P);
    float at = 0.f;
    for (long i = 0; i < l.P; ++i) {
      l.w[i] = rnd();
      l.deltas[i] = rnd() / 32.f;
      l.t[i] = sorted ? (at += rnd() / 32.f) : rnd();
    }
    for (long i = 0; i < l.P; i += 7) l.w[i] = NAN;
    for (long i = 3; i < l.P; i += 11) l.w[i] = -1.f;
    for (long i = 5; i < l.P; i += 13) l.w[i] = 0.f;
    l.w[l.P - 2] = INFINITY;
    return l;
  };
  std::vector<float> dir(3 * R), g_loss(R);
  for (long i = 0; i < 3 * R; ++i) dir[i] = rnd() - 0.5f;
  dir[9] = dir[10] = dir[11] = 0.f;  // ray 3: |dir| = 0
  for (long r = 0; r < R; ++r) g_loss[r] = rnd() - 0.5f;
  for (int variant = 0; variant < 3; ++variant) {  // a monotone envelope; a random one; a random one with NaN and infinite t
    List e = make(len_e, variant == 0), f = make(len_f, true);
    if (variant == 2) {
      for (long i = 1; i < e.P; i += 9) e.t[i] = NAN;
      e.t[e.P / 2] = INFINITY, f.t[f.P / 2] = NAN, f.deltas[f.P / 3] = INFINITY;
    }
    const float epss[2] = {0.f, 1.1920929e-7f};
    for (float eps : epss) {
      std::vector<float> lo(e.P, -7.5f), hi(e.P, -7.5f), cdf(e.P, -7.5f), coef(f.P, -7.5f), loss(R, -7.5f), g_w_e(e.P, -7.5f);
      std::vector<int32_t> span(2 * f.P, -7);
      proposal_host_envelope(e.w.data(), e.t.data(), e.deltas.data(), e.start.data(), e.count.data(), dir.data(), R, e.P, lo.data(), hi.data(), cdf.data());
      proposal_host_forward(lo.data(), hi.data(), cdf.data(), e.start.data(), e.count.data(), e.P, f.w.data(), f.t.data(), f.deltas.data(), f.start.data(),
                            f.count.data(), f.P, dir.data(), R, eps, span.data(), coef.data(), loss.data());
      proposal_host_backward(g_loss.data(), span.data(), coef.data(), e.w.data(), e.start.data(), e.count.data(), e.P, f.start.data(), f.count.data(), f.P, R,
                             g_w_e.data());
      for (long r = 0; r < R; ++r) {
        const lab4d_prune::Rows re = lab4d_prune::rows_of(e.start.data(), e.count.data(), r, e.P);
        const lab4d_prune::Rows rf = lab4d_prune::rows_of(f.start.data(), f.count.data(), r, f.P);
        for (long i = rf.s; i < rf.s + rf.n; ++i) {
          if (span[2 * i] < 0 || span[2 * i] > re.n || span[2 * i + 1] < 0 || span[2 * i + 1] > re.n) return fail("a span outside [0, n_e]");
          if (!(coef[i] <= 0.f) && i != f.P - 2) return fail("a coefficient that is positive or NaN");  // (row P - 2: the infinite fine weight, inf / inf)
        }
        if (!(loss[r] >= 0.f) && r != R - 2) return fail("a loss that is negative or NaN");  // (ray R - 2 owns that row)
        if (rf.n == 0 && loss[r] != 0.f) return fail("a ray without fine rows must cost nothing");
        for (long j = re.s; j < re.s + re.n; ++j)
          if (!(e.w[j] > 0.f) && g_w_e[j] != 0.f) return fail("a gradient on a weight that is not > 0");
      }
      if (loss[R - 1] != 0.f || span[0] != 0 || span[1] != 0) return fail("an empty envelope must give empty spans");
    }
    // the weights adjoint on the same list, density = its weights scaled (NaN, negative, infinite), with and without g_trans
    std::vector<float> dens(e.P), g_w(e.P), g_trans(R), g_density(e.P, -7.5f);
    for (long i = 0; i < e.P; ++i) dens[i] = 40.f * e.w[i], g_w[i] = rnd() - 0.5f;
    for (long r = 0; r < R; ++r) g_trans[r] = rnd() - 0.5f;
    proposal_host_weights_backward(dens.data(), e.deltas.data(), e.start.data(), e.count.data(), R, e.P, g_w.data(), g_trans.data(), g_density.data());
    proposal_host_weights_backward(dens.data(), e.deltas.data(), e.start.data(), e.count.data(), R, e.P, g_w.data(), nullptr, g_density.data());
    for (long i = 0; i < e.P; ++i)
      if (!(dens[i] * e.deltas[i] > 0.f) && g_density[i] != 0.f && g_density[i] != -7.5f) return fail("a gradient on a row whose tau does not count");
  }
  // no rays, and no rows (null data pointers: nothing may be touched)
  proposal_host_weights_backward(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr);
  proposal_host_envelope(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr);
  proposal_host_forward(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, 1e-7f, nullptr, nullptr, nullptr);
  proposal_host_backward(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, nullptr);
  std::vector<int32_t> s2 = {0, 4}, c2 = {3, 1};
  std::vector<float> d2(6, 1.f), loss2(2, -7.5f), g2(2, 1.f);
  proposal_host_envelope(nullptr, nullptr, nullptr, s2.data(), c2.data(), d2.data(), 2, 0, nullptr, nullptr, nullptr);
  proposal_host_forward(nullptr, nullptr, nullptr, s2.data(), c2.data(), 0, nullptr, nullptr, nullptr, s2.data(), c2.data(), 0, d2.data(), 2, 1e-7f, nullptr, nullptr,
                        loss2.data());
  proposal_host_backward(g2.data(), nullptr, nullptr, nullptr, s2.data(), c2.data(), 0, s2.data(), c2.data(), 0, 2, nullptr);
  proposal_host_weights_backward(nullptr, nullptr, s2.data(), c2.data(), 2, 0, nullptr, nullptr, nullptr);
  if (loss2[0] != 0.f || loss2[1] != 0.f) return fail("P = 0");
  printf("proposal_host_main: ok\n");
  return 0;
}
