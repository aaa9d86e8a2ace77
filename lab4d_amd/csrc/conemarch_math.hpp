// Cascaded occupancy grids and cone-stepped packed marching of the hash field (csrc/conemarch.hip; contract: include/lab4d_conemarch.h): the
// step of a ray grows with the distance, dt = clamp(t * cone_angle, dt_min, dt_max), and every sample is looked up in the level of a cascade
// of K occupancy grids -- each twice the extent of the one before around the same centre -- that fits its position and its step
// (Mueller et al. 2022, appendix E; nerfacc ships the same pair).  The reference has no counterpart (nnutils/nerf.py:98 is a TODO), so the
// rules below are this repository's own.
// Plain C++ behind LAB4D_HD over the helpers of occgrid_math.hpp (to_x01, cell_of_point, sample_mask, bit_of, mul_rn / add_rn / div_rn) and of
// ray_math.hpp (clip_ray, dir_length, point_at): no new clip, no new cell rule, no new |d|.  The kernels run these functions one lane per
// ray / point, tests/host_harness/conemarch/conemarch_host.cpp compiles them with g++ (-ffp-contract=off) as serial loops, and the GPU suite
// holds the kernels word for word to that twin.
//
// CASCADE  K levels, 1 <= K <= 8; one G for all levels, 2 <= G <= 256, even when K > 1.  aabbs (K, 6) fp32, level c = {lo xyz, hi xyz},
//          taken as given; bits (K, n_words(G)), each level in the layout of occgrid_math.hpp's GRID.
// EDGE     edge_c = the minimum over the three axes of div_rn(hi - lo, (float)G).
// LEVEL    of a point p with a step of world length delta:  c_pos = the smallest c for which p has a cell in box c (cell_of_point >= 0);
//          none: the point is not kept.  c_step = the smallest c with delta <= edge_c; none: K - 1.  level = max(c_pos, c_step).  The point
//          is kept iff sample_mask(p, aabbs[level], bits[level], G).
// STEPS    ray o + t d, t in [t0, t1], d of any length.  clip_ray against box K - 1 gives [t_in, t_out] within [t0, t1]; a miss, a
//          non-finite o, d, t0 or t1, or t0 > t1: count 0.  a_0 = t_in;  s_k = min(max(mul_rn(a_k, cone), dt_min), dt_max);
//          t_k = add_rn(a_k, mul_rn(0.5f, s_k));  a_{k+1} = add_rn(a_k, s_k).  Candidate k exists while k < k_max and t_k <= t_out; the walk
//          ends at the first k that fails.  The recurrence IS the definition: it accumulates by nature, and it is deterministic because every
//          operation is rounded on its own.  p_k = point_at(o, d, t_k), delta_k = mul_rn(s_k, |d|).
// PER ROW  t = t_k, steps = s_k, deltas = delta_k, xyz = p_k, dirs = d / |d| (as the march of packed_math.hpp writes it), ray_idx, level.
// LAYOUT   packed_math.hpp's, word for word: ray order, ascending k within a ray; count, the caller's exclusive scan, write; a STATIC cap;
//          ray_count_out clamped, total untruncated, overflow = total > cap.  Rows in [min(total, cap), cap) are parked with the park point
//          of box K - 1: dirs = (0, 0, 1), t = steps = deltas = 0, ray_idx = level = -1.  No atomics.
#pragma once
#include "packed_math.hpp"

namespace lab4d_cone {
namespace occ = lab4d_occ;
using lab4d_packed::clamp_count;
using lab4d_packed::park_point;
using lab4d_ray::clip_ray;
using lab4d_ray::dir_length;
using lab4d_ray::point_at;

constexpr int kMinK = 1, kMaxK = 8;

// EDGE of every level; the entries behind K are never looked at.  (Read and written with constant indices only, in fully unrolled loops: on
// the device the eight values stay in registers.)
struct Edges {
  float e[kMaxK];
};

LAB4D_HD float level_edge(const float* aabb, int G) {
  const float g = (float)G;
  const float ex = occ::div_rn(aabb[3] - aabb[0], g), ey = occ::div_rn(aabb[4] - aabb[1], g), ez = occ::div_rn(aabb[5] - aabb[2], g);
  const float m = ex < ey ? ex : ey;
  return m < ez ? m : ez;
}

LAB4D_HD Edges cascade_edges(const float* aabbs, int K, int G) {
  Edges E;
#pragma unroll
  for (int c = 0; c < kMaxK; ++c) E.e[c] = c < K ? level_edge(aabbs + 6 * c, G) : 0.f;
  return E;
}

// c_step: the smallest c with delta <= edge_c, K - 1 if there is none (a NaN delta: none)
LAB4D_HD int step_level(float delta, const Edges& E, int K) {
  int c_step = K - 1;
#pragma unroll
  for (int c = kMaxK - 1; c >= 0; --c)
    if (c < K && delta <= E.e[c]) c_step = c;
  return c_step;
}

// c_pos: the smallest c for which p has a cell in box c, -1 if there is none
LAB4D_HD int pos_level(const float* p, const float* aabbs, int K, int G) {
  for (int c = 0; c < K; ++c)
    if (occ::cell_of_point(p, aabbs + 6 * c, G) >= 0) return c;
  return -1;
}

// LEVEL: *level = max(c_pos, c_step), -1 where the point has no cell in any box; returns kept
LAB4D_HD bool cascade_keep(const float* p, float delta, const float* aabbs, const uint32_t* bits, const Edges& E, int K, int G, int* level) {
  const int c_pos = pos_level(p, aabbs, K, G);
  *level = -1;
  if (c_pos < 0) return false;
  const int c_step = step_level(delta, E, K);
  const int c = c_pos > c_step ? c_pos : c_step;
  *level = c;
  return occ::sample_mask(p, aabbs + 6 * c, bits + (long)c * occ::n_words(G), G);
}

LAB4D_HD float cone_step(float a, float cone, float dt_min, float dt_max) {
  const float x = occ::mul_rn(a, cone);
  const float lo = x > dt_min ? x : dt_min;
  return lo < dt_max ? lo : dt_max;
}

// STEPS.  Calls keep(i, t_k, s_k, delta_k, p_k, level) for the ray's kept candidates in ascending k (i = 0, 1, ...: the row's place within the
// ray) and returns their number.
template <class Keep>
LAB4D_HD int march_cone_ray(const float* o, const float* d, float t0, float t1, const float* aabbs, const uint32_t* bits, const Edges& E, int K, int G,
                            float cone, float dt_min, float dt_max, int k_max, Keep&& keep) {
  float t_in, t_out, len;
  if (clip_ray(o, d, t0, t1, aabbs + 6 * (K - 1), &t_in, &t_out, &len) != 2) return 0;
  float a = t_in;
  int n = 0;
  for (int k = 0; k < k_max; ++k) {
    const float s = cone_step(a, cone, dt_min, dt_max);
    const float t = occ::add_rn(a, occ::mul_rn(0.5f, s));
    if (!(t <= t_out)) break;
    float p[3];
    point_at(o, d, t, p);
    const float delta = occ::mul_rn(s, len);
    int level;
    if (cascade_keep(p, delta, aabbs, bits, E, K, G, &level)) keep(n++, t, s, delta, p, level);
    a = occ::add_rn(a, s);
  }
  return n;
}

}  // namespace lab4d_cone
