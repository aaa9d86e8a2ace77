// CPU twin of lab4d_amd/csrc/pmerge.hip: serial loops over the SAME functions (csrc/pmerge_math.hpp over csrc/prune_math.hpp and
// csrc/packed_math.hpp) with the layout of include/lab4d_pmerge.h.  Built by tests/host_twin.py with g++ -ffp-contract=off;
// tests/test_pmerge_host.py pins it against numpy's stable argsort, the GPU suite holds the kernels word for word to it
// (tests/test_gpu_zzzzzzzzzzzzzpmerge.py).
#include <stdint.h>

#include "pmerge_math.hpp"

namespace pk = lab4d_packed;
namespace pm = lab4d_pmerge;

extern "C" void pmerge_host_count(const int32_t* start_a, const int32_t* count_a, long Pa, const int32_t* start_b, const int32_t* count_b, long Pb, long R,
                                  int32_t* ray_count) {
  for (long ray = 0; ray < R; ++ray) ray_count[ray] = pm::rows_of(start_a, count_a, ray, Pa).n + pm::rows_of(start_b, count_b, ray, Pb).n;
}

// the rows of one list of one ray
static void merge_rows_of(bool from_b, const float* t_mine, const float* deltas_mine, pm::Rows mine, const float* t_other, pm::Rows other, long Pa, long ray,
                          long base, long cap, float* t, float* deltas, int32_t* ray_idx, int32_t* src, int32_t* pos_mine) {
  for (int i = 0; i < mine.n; ++i) {
    const long row = mine.s + i;
    const float x = t_mine[row];
    const long dst = base + (from_b ? pm::place_b(i, x, t_other + other.s, other.n) : pm::place_a(i, x, t_other + other.s, other.n));
    if (dst < 0 || dst >= cap) continue;
    t[dst] = x;
    deltas[dst] = deltas_mine[row];
    ray_idx[dst] = (int32_t)ray;
    src[dst] = pm::src_of(from_b, row, Pa);
    pos_mine[row] = (int32_t)dst;
  }
}

// ray_start: the exclusive prefix sum of pmerge_host_count's counts
extern "C" void pmerge_host_write(const float* t_a, const float* deltas_a, const int32_t* start_a, const int32_t* count_a, long Pa, const float* t_b,
                                  const float* deltas_b, const int32_t* start_b, const int32_t* count_b, long Pb, long R, const int32_t* ray_start, long cap,
                                  float* t, float* deltas, int32_t* ray_idx, int32_t* src, int32_t* pos_a, int32_t* pos_b, int32_t* ray_count_out,
                                  int32_t* total, uint8_t* overflow) {
  for (long row = 0; row < Pa; ++row) pos_a[row] = -1;
  for (long row = 0; row < Pb; ++row) pos_b[row] = -1;
  long tot = 0;
  for (long ray = 0; ray < R; ++ray) {
    const pm::Rows ra = pm::rows_of(start_a, count_a, ray, Pa), rb = pm::rows_of(start_b, count_b, ray, Pb);
    const long base = ray_start[ray];
    merge_rows_of(false, t_a, deltas_a, ra, t_b, rb, Pa, ray, base, cap, t, deltas, ray_idx, src, pos_a);
    merge_rows_of(true, t_b, deltas_b, rb, t_a, ra, Pa, ray, base, cap, t, deltas, ray_idx, src, pos_b);
    const int n = ra.n + rb.n;
    ray_count_out[ray] = pk::clamp_count((int)base, n, (int)cap);
    tot = base + n;
  }
  *total = (int32_t)tot;
  *overflow = tot > cap ? 1 : 0;
  for (long row = tot < 0 ? 0 : tot; row < cap; ++row) {
    t[row] = 0.f;
    deltas[row] = 0.f;
    ray_idx[row] = -1;
    src[row] = -1;
  }
}

extern "C" void pmerge_host_gather(const float* a, long Pa, const float* b, long Pb, const int32_t* idx, long n, int C, float* out) {
  for (long j = 0; j < n; ++j)
    for (int c = 0; c < C; ++c) out[j * C + c] = pm::gather_value(a, Pa, b, Pb, idx[j], C, c);
}
