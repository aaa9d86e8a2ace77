// Pruning of a packed sample list by transmittance and opacity (csrc/prune.hip; contract: include/lab4d_prune.h): after the march
// (packed_math.hpp) and a density pass without gradients, the rows BEHIND the surface are dropped before the differentiable field runs --
// the two-pass form of Mueller et al. 2022 (section 5.4 / appendix E) and of nerfacc.  The reference has no counterpart; the rules are this
// repository's own.  Plain C++ behind LAB4D_HD: the kernels run these functions one wave per ray, tests/host_harness/prune/prune_host.cpp compiles
// them with g++ (-ffp-contract=off) around a serial emulation of the 64-lane scan, and the GPU suite holds the kernels word for word to
// that twin.
//
// ROWS     ray r owns rows ray_start[r] .. ray_start[r] + ray_count[r] - 1 of a packed list with P rows; a (start, count) that leaves
//          [0, P) is cut to it (rows_of, the rule of packed.hip).
// TAU      tau_i = mul_rn(density_i, deltas_i); a tau that is NaN or not > 0 counts as 0 (the occupancy grid's rule for densities).
// PREFIX   the exclusive prefix E_i of tau along the ray, in fp32, in ONE order: rows in chunks of 64 from the ray's first row; inside a
//          chunk the doubling scan of wave_scan_incl (common.hpp): for o = 1, 2, 4 .. 32: v[l] += v[l - o] for l >= o, plain fp32 adds,
//          dead lanes hold 0; then + carry, the inclusive value of the previous chunk's lane 63 (0 for the first chunk).  E_i is the
//          inclusive value of the lane before, carry itself for lane 0.  (What chunk_weights of packed.hip computes.)
// STOP     j* = the first row of the ray with E_j > tau_stop: the chunks in order, the lowest lane inside a chunk (a ballot), so the stop
//          is monotone by construction even where an fp32 prefix dips by an ulp.  Every row >= j* is dropped.  tau_stop = +inf never stops.
// OPACITY  a row before the stop is kept iff tau_i >= tau_min (tau_min = 0 keeps all of them).  Dropped rows still count in the prefix of
//          the rows behind them: transmittance is a property of the ray, not of the kept set.
//          No exp anywhere: the caller converts tau_stop = -log(early_stop_eps), tau_min = -log1p(-alpha_thre) in double precision.
// LAYOUT   the march's: survivors in ray order, ascending row within a ray; new_count[r] survivors, new_start its exclusive prefix sum,
//          total the sum; a STATIC capacity cap: rows >= cap are not written, the emitted count is clamp(cap - new_start, 0, new_count),
//          overflow = total > cap, total untruncated; rows in [min(total, cap), cap) are parked as the march parks them (park_point of
//          packed_math.hpp, dirs (0, 0, 1), ray_idx -1, t = deltas = 0) with src_row = -1.  A survivor copies t, deltas, xyz, dirs bit for
//          bit; ray_idx = its ray, src_row = its source row.
#pragma once
#include "packed_math.hpp"

namespace lab4d_prune {
using lab4d_rn::mul_rn;

struct Rows {
  long s;
  int n;
};
LAB4D_HD Rows rows_of(const int32_t* ray_start, const int32_t* ray_count, long ray, long P) {
  const long s = ray_start[ray];
  long n = ray_count[ray];
  if (s < 0 || s >= P || n <= 0) return {0, 0};
  if (n > P - s) n = P - s;
  return {s, (int)n};
}

LAB4D_HD float tau_of(float density, float delta) {
  const float tau = mul_rn(density, delta);
  return tau > 0.f ? tau : 0.f;  // (NaN compares false)
}

// the lane's vote for the stop; the lowest voting lane of the first chunk with a vote is j*
LAB4D_HD bool stops(bool live, float excl, float tau_stop) { return live && excl > tau_stop; }

// the lowest set bit of a chunk's ballot, 64 without one
LAB4D_HD int first_lane(uint64_t ballot) { return ballot ? __builtin_ctzll(ballot) : 64; }

LAB4D_HD bool keeps(bool live, int lane, int stop_lane, float tau, float tau_min) { return live && lane < stop_lane && tau >= tau_min; }

// lanes below `lane` in a ballot: a survivor's place among its chunk's survivors
LAB4D_HD int rank_of(uint64_t ballot, int lane) { return __builtin_popcountll(ballot & ((1ull << lane) - 1ull)); }

}  // namespace lab4d_prune
