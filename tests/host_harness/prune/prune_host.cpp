// CPU twin of lab4d_amd/csrc/prune.hip: serial loops over the SAME functions (csrc/prune_math.hpp over csrc/packed_math.hpp) with the layout
// of include/lab4d_prune.h.  A wave is emulated as 64 array entries: the doubling scan of wave_scan_incl (common.hpp) step by step, the
// ballots as 64-bit words.  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_prune_host.py pins it against numpy in float64,
// the GPU suite holds both kernels word for word to it (tests/test_gpu_zzzzzzzzprune.py).
#include <stdint.h>

#include "prune_math.hpp"

namespace pk = lab4d_packed;
namespace pr = lab4d_prune;

// wave_scan_incl over all 64 lanes at once: every step reads the values of the step before
static void scan_incl(float* v) {
  for (int o = 1; o < 64; o <<= 1) {
    float before[64];
    for (int l = 0; l < 64; ++l) before[l] = v[l];
    for (int l = o; l < 64; ++l) v[l] = before[l] + before[l - o];
  }
}

// keep (P): rows of no ray are left as they are
extern "C" void prune_host_count(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P, float tau_stop,
                                 float tau_min, uint8_t* keep, int32_t* new_count) {
  for (long ray = 0; ray < R; ++ray) {
    const pr::Rows rr = pr::rows_of(ray_start, ray_count, ray, P);
    float carry = 0.f;
    int kept = 0, j0 = 0;
    bool stopped = false;
    for (; j0 < rr.n && !stopped; j0 += 64) {
      float tau[64], incl[64];
      for (int l = 0; l < 64; ++l) incl[l] = tau[l] = j0 + l < rr.n ? pr::tau_of(density[rr.s + j0 + l], deltas[rr.s + j0 + l]) : 0.f;
      scan_incl(incl);
      uint64_t stop = 0;
      for (int l = 0; l < 64; ++l) {
        incl[l] += carry;
        const float excl = l == 0 ? carry : incl[l - 1];
        if (pr::stops(j0 + l < rr.n, excl, tau_stop)) stop |= 1ull << l;
      }
      carry = incl[63];
      const int stop_lane = pr::first_lane(stop);
      for (int l = 0; l < 64 && j0 + l < rr.n; ++l) {
        const bool k = pr::keeps(true, l, stop_lane, tau[l], tau_min);
        keep[rr.s + j0 + l] = k ? 1 : 0;
        kept += k;
      }
      stopped = stop != 0;
    }
    for (long i = j0; i < rr.n; ++i) keep[rr.s + i] = 0;
    new_count[ray] = kept;
  }
}

// new_start: the exclusive prefix sum of prune_host_count's counts
extern "C" void prune_host_write(const uint8_t* keep, const int32_t* ray_start, const int32_t* ray_count, const int32_t* new_start, long R, long P, long cap,
                                 const float* aabb, const float* t, const float* deltas, const float* xyz, const float* dirs, float* t_out, float* deltas_out,
                                 float* xyz_out, float* dirs_out, int32_t* ray_idx_out, int32_t* src_row_out, int32_t* new_count_out, int32_t* total,
                                 uint8_t* overflow) {
  long tot = 0;
  for (long ray = 0; ray < R; ++ray) {
    const pr::Rows rr = pr::rows_of(ray_start, ray_count, ray, P);
    const long base = new_start[ray];
    int n = 0;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      uint64_t bal = 0;
      for (int l = 0; l < 64 && j0 + l < rr.n; ++l)
        if (keep[rr.s + j0 + l] != 0) bal |= 1ull << l;
      for (int l = 0; l < 64; ++l) {
        if (!((bal >> l) & 1ull)) continue;
        const long row = rr.s + j0 + l, dst = base + n + pr::rank_of(bal, l);
        if (dst < 0 || dst >= cap) continue;
        t_out[dst] = t[row];
        deltas_out[dst] = deltas[row];
        for (int a = 0; a < 3; ++a) {
          xyz_out[3 * dst + a] = xyz[3 * row + a];
          dirs_out[3 * dst + a] = dirs[3 * row + a];
        }
        ray_idx_out[dst] = (int32_t)ray;
        src_row_out[dst] = (int32_t)row;
      }
      n += __builtin_popcountll(bal);
    }
    new_count_out[ray] = pk::clamp_count((int)base, n, (int)cap);
    tot = base + n;
  }
  *total = (int32_t)tot;
  *overflow = tot > cap ? 1 : 0;
  float p[3];
  pk::park_point(aabb, p);
  for (long row = tot < 0 ? 0 : tot; row < cap; ++row) {
    t_out[row] = 0.f;
    deltas_out[row] = 0.f;
    for (int a = 0; a < 3; ++a) {
      xyz_out[3 * row + a] = p[a];
      dirs_out[3 * row + a] = a == 2 ? 1.f : 0.f;
    }
    ray_idx_out[row] = -1;
    src_row_out[row] = -1;
  }
}
