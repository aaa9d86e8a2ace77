// The distortion loss of a packed sample list (csrc/distort.hip; contract: include/lab4d_distort.h): the regulariser of Barron et al. 2022
// (mip-NeRF 360, eq. 15) and of nerfacc on the rows of a packed ray.  The reference has no counterpart; the rules are this repository's own.
// Plain C++ behind LAB4D_HD: the kernels run these functions one wave per ray around their chunked scans, and
// tests/host_harness/distort/distort_host.cpp compiles them with g++ (-ffp-contract=off) around serial fp32 prefix sums.  The sums run in
// another order on the two sides, so the kernels are held to the float64 definition and to the twin within the fp32 bar, not word for word
// (the compositing kernels' contract, not the march's).
//
// ROWS     rows_of (prune_math.hpp): the ray's rows, a (start, count) that leaves [0, P) cut to it.
// WEIGHTS  w_i = weight_of(tau_i, sum_{j<i} tau_j), tau_i = density_i * deltas_i; T_i = transmit_of(sum_{j<=i} tau_j) (packed_math.hpp).
// SHIFT    m_i = mid_i - mid_first: the loss only sees differences of midpoints.
// LOSS     loss = sum_i [ 2 w_i (m_i W_i - M_i) + (1/3) w_i^2 width_i ],  W_i = sum_{j<i} w_j,  M_i = sum_{j<i} w_j m_j
//          (= sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 width_i for ascending m).
// ADJOINT  g_w_i = 2 [ (m_i W_i - M_i) + ((M - Mi_i) - m_i (W - Wi_i)) ] + (2/3) w_i width_i with the totals W, M and the inclusive
//          prefixes Wi_i = W_i + w_i, Mi_i = M_i + w_i m_i;  d w_i / d tau_i = T_i and d w_j / d tau_i = -w_j for j > i, so
//          g_tau_i = g_w_i T_i - S_i, S_i = sum_{j>i} g_w_j w_j = 2 loss - (inclusive prefix of g_w w): the loss is homogeneous of degree 2
//          in w.
#pragma once
#include "prune_math.hpp"

namespace lab4d_distort {
using lab4d_prune::Rows;
using lab4d_prune::rows_of;

LAB4D_HD float shifted_mid(float mid, float mid_first) { return mid - mid_first; }

// row i's share of the pair term: w_i against every row in front of it, counted for both orders
LAB4D_HD float pair_term(float w, float m, float W_excl, float M_excl) { return 2.f * w * (m * W_excl - M_excl); }

LAB4D_HD float self_term(float w, float width) { return (1.f / 3.f) * w * w * width; }

// dloss / dw_i: the rows in front of i, the rows behind it, its own width
LAB4D_HD float weight_adjoint(float w, float m, float width, float W_excl, float M_excl, float W_incl, float M_incl, float W_total, float M_total) {
  return 2.f * ((m * W_excl - M_excl) + ((M_total - M_incl) - m * (W_total - W_incl))) + (2.f / 3.f) * w * width;
}

// S_i from the ray's loss and the inclusive prefix of g_w w
LAB4D_HD float suffix_of(float loss, float gww_incl) { return 2.f * loss - gww_incl; }

// dloss / dtau_i; T_incl = exp(-sum_{j<=i} tau_j)
LAB4D_HD float tau_adjoint(float g_w, float T_incl, float S) { return g_w * T_incl - S; }

}  // namespace lab4d_distort
