// Importance resampling of a packed sample list per ray (csrc/presample.hip; contract: include/lab4d_presample.h): the coarse-to-fine step of
// the reference's renderer -- NeRF.importance_sampling (nnutils/nerf.py:686-738): compute_weights of a coarse pass without gradients, then the
// fine depths by inverse CDF (render_utils.sample_pdf, utils/render_utils.py:187-233) -- for a packed list, whose rays have their own lengths.
// The reference has no packed lists: the rules are this repository's own.  Plain C++ behind LAB4D_HD: the kernels run these functions one
// wave per ray, tests/host_harness/presample/presample_host.cpp compiles them with g++ (-ffp-contract=off) around a serial emulation of the
// 64-lane scans, and the GPU suite holds both resample kernels word for word to that twin.  (The weights call evaluates expf, whose last
// bits differ between the two sides: it is held to float64 instead, and the resample kernels take the weights as an input and call no exp.)
//
// ROWS     rows_of (prune_math.hpp): ray r owns rows ray_start[r] .. + ray_count[r] of a list with P rows, cut to [0, P).  n: the cut count.
// WEIGHTS  tau_i = tau_of (prune_math.hpp: NaN or not > 0 counts as 0); E_i = the exclusive prefix of tau in the PREFIX order of
//          lab4d_prune.h (chunks of 64, doubling scan, carry); w_i = weight_of(tau_i, E_i), trans = transmit_of(the inclusive value of the
//          ray's last row) (packed_math.hpp), 1 for a ray without rows.
// MASS     m_i = add_rn(max(w_i, 0), eps), a NaN weight counting as 0 (mass_of).  C_i / E_i: the inclusive / exclusive prefix of m along the
//          ray in the same PREFIX order; E_i is C_{i-1}, 0 for the ray's first row.  W = C of the ray's last row, 0 for a ray without rows.
// COUNT    new_count[r] = n_imp if n > 0 and W > 0, else 0 (count_of).
// QUERY    u_k = div_rn(k + 0.5f, n_imp) (query_u), or the caller's u[r * n_imp + k] clamped to [0, 1] with NaN -> 0 (clamp01): meant to be
//          non-decreasing per ray.  q_k = mul_rn(u_k, W).
// ROW      i_k = min(count_before(C, n, q_k, or_equal), n - 1) (row_of over pmerge_math.hpp's search: no second loop).  Where C is monotone
//          that is the first row with C_i > q_k; where an fp32 prefix dips by an ulp, or C holds inf, the search still ends after
//          ceil(log2(n + 1)) steps with a value in range.
// PLACE    f = clamp01(div_rn(q_k - E_i, m_i)) (place_f; 0 / 0 -> 0).  The row's interval in t is centred on t_i and has the width
//          div_rn(deltas_i, |dir_r|), |dir| = dir_length (ray_math.hpp), what the march multiplied dt by; 0 for |dir| = 0 (width_of).
//          t'_k = add_rn(t_i, mul_rn(f - 0.5f, width)) (t_of).
// ORDER    the emitted t_k = the running maximum of t' over k' <= k within the ray (later_of, scanned 64 samples at a time with a carry):
//          non-decreasing in t whatever the input, the precondition of the merge.  (max is associative: no order needs stating; both sides
//          still run the same doubling scan, so that even the sign of a zero agrees.)
// SPAN     deltas_k = min(deltas_i, div_rn(mul_rn(deltas_i, W), mul_rn(n_imp, m_i))) (span_of): the length along the ray that carries 1 / n_imp
//          of the mass, never more than the source row's own; a quotient that is NaN gives deltas_i.
// PER ROW  xyz = point_at(o, d, t_k); dirs = d / |d| per component as the march writes it (0 for |d| = 0); ray_idx = r; src_row = the global
//          index of source row i_k.
// LAYOUT   the march's: new_start = the exclusive prefix sum of new_count (the caller's scan), total = the sum, untruncated; a STATIC
//          capacity cap: rows >= cap are not written, the emitted count is clamp_count, overflow = total > cap; rows in [min(total, cap), cap)
//          are parked at park_point(aabb) with dirs (0, 0, 1), t = deltas = 0, ray_idx = src_row = -1.  No atomics.
#pragma once
#include "pmerge_math.hpp"

namespace lab4d_presample {
using lab4d_pmerge::count_before;
using lab4d_prune::Rows;
using lab4d_prune::rows_of;
using lab4d_prune::tau_of;
using lab4d_rn::add_rn;
using lab4d_rn::div_rn;
using lab4d_rn::mul_rn;

LAB4D_HD float clamp01(float v) { return v > 0.f ? (v < 1.f ? v : 1.f) : 0.f; }  // (NaN compares false: 0)

LAB4D_HD float mass_of(float w, float eps) { return add_rn(w > 0.f ? w : 0.f, eps); }

LAB4D_HD int count_of(int n, float W, int n_imp) { return n > 0 && W > 0.f ? n_imp : 0; }

LAB4D_HD float query_u(int k, int n_imp) { return div_rn((float)k + 0.5f, (float)n_imp); }

// C: the ray's n >= 1 inclusive prefixes
LAB4D_HD int row_of(const float* C, int n, float q) {
  const int i = count_before(C, n, q, true);
  return i < n - 1 ? i : n - 1;
}

LAB4D_HD float place_f(float q, float excl, float m) { return clamp01(div_rn(add_rn(q, -excl), m)); }

LAB4D_HD float width_of(float delta, float len) { return len > 0.f ? div_rn(delta, len) : 0.f; }

LAB4D_HD float t_of(float t_i, float f, float width) { return add_rn(t_i, mul_rn(add_rn(f, -0.5f), width)); }

LAB4D_HD float span_of(float delta, float W, int n_imp, float m) {
  const float s = div_rn(mul_rn(delta, W), mul_rn((float)n_imp, m));
  return s < delta ? s : delta;
}

// the running maximum: `before` is the value of the earlier samples
LAB4D_HD float later_of(float before, float v) { return before > v ? before : v; }

}  // namespace lab4d_presample
