// Proposal (interval, outer-measure) loss between two packed sample lists per ray, and the adjoint of the compositing weights of a packed
// list (csrc/proposal.hip; contract: include/lab4d_proposal.h): the two pieces a TRAINED proposal field needs, the scheme of Barron et al.
// 2022 (mip-NeRF 360, section 3 and equation 13) -- a cheap field is taught to put its weights where the main field's are, by a loss that
// makes the proposal list's weights an upper envelope of the fine list's weights.  The reference has neither and no packed lists: the rules
// are this repository's own.  Plain C++ behind LAB4D_HD: the kernels run these functions one wave per ray,
// tests/host_harness/proposal/proposal_host.cpp compiles them with g++ (-ffp-contract=off) around a serial emulation of the 64-lane scan,
// and the GPU suite holds the envelope, forward and backward kernels word for word to that twin.  (The weights adjoint evaluates expf, whose
// last bits differ between the two sides: it is held to float64 instead.)
//
// Both lists share the R rays and dir (R, 3).  The envelope list e has Pe rows and weights w_e, the fine list f has Pf rows and weights w_f.
//
// ROWS      rows_of (prune_math.hpp) for each list: a (start, count) that leaves [0, P) is cut to it.  n_e, n_f: the cut counts.
// INTERVAL  h_i = mul_rn(0.5f, div_rn(deltas_i, |dir_r|)) (half_of over presample_math.hpp's width_of: |dir| = dir_length, 0 for |dir| = 0);
//           lo_i = sub_rn(t_i, h_i), hi_i = add_rn(t_i, h_i).  The envelope's lo and hi are meant to be non-decreasing per ray (marched and
//           pruned lists are); the fine list has no such condition (a resampled list is not monotone in lo).
// MASS      m_j = max(w_e_j, 0), a NaN counting as 0 (pos_of).  C_j: its inclusive prefix along the ray in the PREFIX order of lab4d_prune.h
//           (chunks of 64, doubling scan, carry).
// SPAN      j0_i = count_before(hi_e, n_e, lo_i, true), j1_i = count_before(lo_e, n_e, hi_i, false) (pmerge_math.hpp's search: no new
//           loop).  The envelope rows that overlap fine row i with positive length are [j0, j1), indices within the ray; the span is empty
//           when j1 <= j0.  Whatever the input (NaN, a non-monotone envelope), both indices lie in [0, n_e].
// BOUND     B_i = sub_rn(C[j1 - 1], j0 > 0 ? C[j0 - 1] : 0), 0 for an empty span, and 0 where that difference is negative (bound_of): the
//           doubling scan adds in another order for every lane, so across rows of no mass an fp32 prefix can dip by an ulp; a fine row
//           of weight 0 would then have the excess of that ulp, divided by eps alone (measured on the test lists without the cut: one
//           fine row in 200, |c| up to 128 at eps = 2^-23, an infinite loss at eps = 0).
// LOSS      v_i = max(w_f_i, 0), a NaN counting as 0; x_i = max(sub_rn(v_i, B_i), 0) (excess_of; a NaN difference counts as 0);
//           l_i = div_rn(mul_rn(x_i, x_i), add_rn(v_i, eps)), exactly 0 when x_i == 0 (loss_of: also for v + eps == 0);
//           c_i = div_rn(mul_rn(-2, x_i), add_rn(v_i, eps)) = dl_i / dB_i, 0 when x_i == 0 (coef_of).
//           loss[r] = the last inclusive value of the PREFIX scan of l over the ray's fine rows, 0 for a ray without fine rows.
// ADJOINT   g_e_j = the sum over i in ascending order with j0_i <= j < j1_i of mul_rn(g_loss[r], c_i), accumulated with add_rn from 0
//           (accumulate), for w_e_j > 0; 0 for a row whose weight is not > 0 (a selection, not a product: gate).  No gradient reaches w_f:
//           mip-NeRF 360 stops it.  No atomics: the result does not depend on scheduling.
// WEIGHTS ADJOINT  for w_i = weight_of(tau_i, E_i) (presample_math.hpp's WEIGHTS):
//           g_tau_i = g_w_i * transmit_of(E_i + tau_i) - (S - S_i) - g_trans[r] * trans[r] (g_tau_of), S_i the inclusive PREFIX scan of
//           g_w_k * w_k and S its last value; g_density_i = g_tau_i * deltas_i where tau_of counted the row (counted), otherwise 0.  A NaN
//           in g_w propagates to the ray's rows.
#pragma once
#include "presample_math.hpp"

namespace lab4d_proposal {
using lab4d_pmerge::count_before;
using lab4d_presample::width_of;
using lab4d_prune::Rows;
using lab4d_prune::rows_of;
using lab4d_prune::tau_of;
using lab4d_rn::add_rn;
using lab4d_rn::div_rn;
using lab4d_rn::mul_rn;

LAB4D_HD float sub_rn(float a, float b) { return add_rn(a, -b); }

LAB4D_HD float pos_of(float w) { return w > 0.f ? w : 0.f; }  // (NaN compares false: 0)

LAB4D_HD float half_of(float delta, float len) { return mul_rn(0.5f, width_of(delta, len)); }
LAB4D_HD float lo_of(float t, float h) { return sub_rn(t, h); }
LAB4D_HD float hi_of(float t, float h) { return add_rn(t, h); }

struct Span {
  int j0, j1;
};
// lo_e, hi_e: the ray's n_e envelope rows
LAB4D_HD Span span_of(const float* lo_e, const float* hi_e, int n_e, float lo, float hi) {
  return {count_before(hi_e, n_e, lo, true), count_before(lo_e, n_e, hi, false)};
}

// C: the ray's n_e inclusive prefixes of the mass
LAB4D_HD float bound_of(const float* C, Span s) {
  if (s.j1 <= s.j0) return 0.f;
  const float B = sub_rn(C[s.j1 - 1], s.j0 > 0 ? C[s.j0 - 1] : 0.f);
  return B < 0.f ? 0.f : B;  // (a NaN stays: the excess then counts as 0)
}

LAB4D_HD float excess_of(float v, float B) { return pos_of(sub_rn(v, B)); }
LAB4D_HD float loss_of(float x, float v, float eps) { return x > 0.f ? div_rn(mul_rn(x, x), add_rn(v, eps)) : 0.f; }
LAB4D_HD float coef_of(float x, float v, float eps) { return x > 0.f ? div_rn(mul_rn(-2.f, x), add_rn(v, eps)) : 0.f; }

LAB4D_HD float accumulate(float acc, float g_loss, float c, int j, int j0, int j1) { return j0 <= j && j < j1 ? add_rn(acc, mul_rn(g_loss, c)) : acc; }
LAB4D_HD float gate(float w_e, float acc) { return w_e > 0.f ? acc : 0.f; }

// ---- the adjoint of the compositing weights -------------------------------------------------------------------------------------------
LAB4D_HD bool counted(float density, float delta) { return mul_rn(density, delta) > 0.f; }
// tail = g_trans[r] * trans[r], 0 without g_trans
LAB4D_HD float g_tau_of(float g_w, float tau, float excl, float S, float S_incl, float tail) {
  return sub_rn(sub_rn(mul_rn(g_w, lab4d_packed::transmit_of(add_rn(excl, tau))), sub_rn(S, S_incl)), tail);
}
LAB4D_HD float g_density_of(float g_tau, float density, float delta) { return counted(density, delta) ? mul_rn(g_tau, delta) : 0.f; }

}  // namespace lab4d_proposal
