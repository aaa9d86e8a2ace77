// Packed ray marching and ragged compositing of the hash field (csrc/packed.hip; contract: include/lab4d_packed.h): a ray is marched at a
// fixed step through the occupied cells of the occupancy bit grid only, the kept samples of all rays form ONE packed list with a per-ray
// (start, count), and that list is composited directly -- Mueller et al. 2022, section 5.4 / appendix E.  The reference has no counterpart
// (nnutils/nerf.py:98 is a TODO), so the rules below are this repository's own; the compositing itself is the reference's compute_weights
// + integrate (utils/render_utils.py:99-160) on every ray alone, at D = the ray's own count.
// Plain C++ behind LAB4D_HD over the helpers of occgrid_math.hpp (to_x01, sample_mask, ray_span, mul_rn / add_rn / div_rn) and over
// ray_math.hpp, where |d| (dir_length) and the point at t (point_at) live for every ray kernel; both keep their names here.  The
// kernels run these functions one lane per ray, tests/host_harness/packed_host.cpp compiles them with g++ (-ffp-contract=off) as serial
// loops, and the GPU suite holds the march kernels word for word to that twin.
//
// MARCH      ray o + t * d, t in [t0, t1], d of any length; a per-call step dt > 0 in the caller's depth units; a per-ray limit k_max >= 1.
//            Candidates sit on the ray's OWN lattice t_k = add_rn(t0, mul_rn(k + 0.5f, dt)) (nothing accumulates), 0 <= k < K,
//            K = min(k_max, number of k with t_k <= t1).  ray_span (occgrid_math.hpp) runs first: a ray that misses keeps nothing, otherwise
//            only the k with t_first <= t_k <= t_last are looked at.  Candidate k is kept iff sample_mask(p_k) is set,
//            p_k[a] = add_rn(o[a], mul_rn(t_k, d[a])): the span only prunes the loop, the per-point bit decides -- exactly what
//            hashfield.forward_compacted(occ=grid) decides for the same point.  Non-finite o, d, t0 or t1, or t0 > t1: count 0.
//            Every kept sample of a ray has delta = mul_rn(dt, |d|), |d| = sqrt of the sum of the three rounded squares (x, then y, then z),
//            and the unit direction d / |d| (correctly rounded division per component).
// LAYOUT     kept samples in ray order, ascending k within a ray.  ray_count[r] = kept samples of ray r, ray_start = its exclusive prefix
//            sum (a scan, never an atomic bump allocator: the layout does not depend on scheduling), total = sum of ray_count.  A STATIC
//            capacity cap bounds the packed buffers: rows >= cap are not written, the emitted count of ray r is
//            clamp(cap - ray_start[r], 0, ray_count[r]), overflow = total > cap, total is the untruncated sum.  Rows in [min(total, cap),
//            cap) are PARKED: a point outside the box (hi + (hi - lo), forward_compacted's rule), direction (0, 0, 1), ray_idx = -1,
//            t = 0, delta = 0.
// COMPOSITE  ray r owns rows ray_start[r] .. + ray_count[r]:  tau_i = density_i * delta_i,  T_i = exp(-sum_{j<=i} tau_j),
//            w_i = (1 - exp(-tau_i)) * exp(-sum_{j<i} tau_j),  mask = sum w.  Field modes as in lab4d_composite_forward: 0 = sum
//            w / (mask + 1e-6) * v, 1 = the same with detached weights, 2 = plain mean over the ray's samples and channels.  A ray
//            without samples: mask = 0 and every output 0 (mode 2 included), no NaN.
#pragma once
#include "occgrid_math.hpp"
#include "ray_math.hpp"

namespace lab4d_packed {
namespace occ = lab4d_occ;
using lab4d_ray::dir_length;  // |d| and o + t * d: ray_math.hpp's, shared with the tracer and the mesh ray caster
using lab4d_ray::point_at;

LAB4D_HD float cand_t(float t0, int k, float dt) { return occ::add_rn(t0, occ::mul_rn((float)k + 0.5f, dt)); }

// the point of a parked row: outside the box on every axis
LAB4D_HD void park_point(const float* aabb, float* p) {
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = occ::add_rn(aabb[3 + a], aabb[3 + a] - aabb[a]);
}

// Calls keep(i, t_k, p_k) for the ray's kept candidates in ascending k (i = 0, 1, ...: the sample's place within the ray) and returns
// their number.  t_k never decreases with k (a rounded product and a rounded sum are monotone), so the loop ends at the first candidate
// behind t1 or the span, and it starts at a candidate that is known to lie before the span (or at 0).
template <class Keep>
LAB4D_HD int march_ray(const float* o, const float* d, float t0, float t1, const float* aabb, const uint32_t* bits, int G, float dt, int k_max,
                       Keep&& keep) {
  float span[2];
  if (!occ::ray_span(o, d, t0, t1, aabb, bits, G, span, nullptr)) return 0;  // (also: non-finite input, t0 > t1, an empty box)
  // a first candidate at or before the span: an estimate, then walked back until it holds (the estimate only saves steps)
  int k = 0;
  {
    const float est = occ::div_rn(span[0] - t0, dt) - 2.f;
    if (est > 0.f) k = est < (float)(k_max - 1) ? (int)est : k_max - 1;
    while (k > 0 && cand_t(t0, k, dt) >= span[0]) --k;
  }
  int n = 0;
  for (; k < k_max; ++k) {
    const float t = cand_t(t0, k, dt);
    if (!(t <= t1) || t > span[1]) break;
    if (t < span[0]) continue;
    float p[3];
    point_at(o, d, t, p);
    if (occ::sample_mask(p, aabb, bits, G)) keep(n++, t, p);
  }
  return n;
}

// the emitted count of a ray under the capacity
LAB4D_HD int clamp_count(int start, int count, int cap) {
  const long room = (long)cap - start;
  return room <= 0 ? 0 : (room < count ? (int)room : count);
}

// ---- compositing ----------------------------------------------------------------------------------------------------------------------
// w_i from tau_i and the exclusive prefix sum of tau; T_i from the inclusive one
LAB4D_HD float weight_of(float tau, float excl) { return (1.f - expf(-tau)) * expf(-excl); }
LAB4D_HD float transmit_of(float incl) { return expf(-incl); }
LAB4D_HD float normaliser(float mask) { return 1.f / (mask + 1e-6f); }

}  // namespace lab4d_packed
