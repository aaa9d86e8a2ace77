/*
 * lab4d_proposal.h -- the proposal (interval, outer-measure) loss between two packed sample lists per ray, forward and adjoint, and the adjoint
 * of the compositing weights of a packed list (included by lab4d_hip.h).
 *
 * lab4d_packed_resample_* (lab4d_presample.h) places the fine rows of a ray where the weights of a coarse pass are.  With a TRAINED proposal
 * field -- Barron et al. 2022 (mip-NeRF 360), section 3 -- the coarse pass is a cheap field of its own, taught by a loss that makes its
 * weights an upper envelope of the main field's weights: every fine interval's weight must be covered by the summed weight of the proposal
 * intervals that overlap it (their equation 13).  That needs the compositing weights of a packed list WITH a backward (lab4d_packed_weights is
 * forward only) and the loss itself on two packed lists whose rays have their own lengths.  The reference has neither and no packed lists, so
 * parity is unpinned by nature and the rules are this repository's own.  The arithmetic is lab4d_amd/csrc/proposal_math.hpp, shared with the
 * CPU twin tests/host_harness/proposal/proposal_host.cpp, to which the envelope, forward and backward kernels are held word for word (they call
 * no exp; the weights adjoint does and is held to float64).
 *
 * Both lists share the R rays and dir (R, 3).  The envelope list e (the proposal's) has Pe rows and weights w_e; the fine list f has Pf rows
 * and weights w_f.
 *
 * Rules:
 *   ROWS      ray r owns rows ray_start[r] .. ray_start[r] + ray_count[r] - 1 of each list; a (start, count) that leaves [0, P) is cut to it
 *             (rows_of of prune_math.hpp).  n_e, n_f are the cut counts.
 *   INTERVAL  h_i = 0.5 * (deltas_i / |dir_r|), the quotient and the product rounded on their own; |dir| as the march forms it for deltas
 *             (lab4d_presample.h, PLACE); the width is 0 for |dir| = 0.  lo_i = t_i - h_i, hi_i = t_i + h_i.  The envelope's lo and hi are
 *             meant to be non-decreasing per ray: marched and pruned lists are.  The fine list has no such condition: a resampled list is
 *             not monotone in lo.
 *   MASS      m_j = max(w_e_j, 0), a NaN counting as 0.  C_j is its inclusive prefix along the ray in the PREFIX order of lab4d_prune.h:
 *             chunks of 64, doubling scan, carry.
 *   SPAN      j0_i = #{j : hi_e_j <= lo_i}, j1_i = #{j : lo_e_j < hi_i}, each by one binary search (count_before of pmerge_math.hpp),
 *             indices within the ray.  The envelope rows that overlap fine row i with positive length are [j0, j1); the span is empty when
 *             j1 <= j0.  Whatever the input, both indices lie in [0, n_e] and the search ends after ceil(log2(n_e + 1)) steps.
 *   BOUND     B_i = C[j1 - 1] - (j0 > 0 ? C[j0 - 1] : 0), one rounded difference; 0 for an empty span, and 0 where the difference is negative:
 *             across rows of no mass an fp32 prefix can dip by an ulp (every lane of the scan adds in its own order), and without the cut a
 *             fine row of weight 0 would carry that ulp as an excess, divided by eps alone.
 *   LOSS      v_i = max(w_f_i, 0), a NaN counting as 0.  x_i = max(v_i - B_i, 0).  l_i = (x_i * x_i) / (v_i + eps), every operation rounded
 *             on its own, exactly 0 when x_i == 0.  c_i = (-2 * x_i) / (v_i + eps) = dl_i / dB_i, 0 when x_i == 0.  loss[r] = the last
 *             inclusive value of the PREFIX scan of l over the ray's fine rows; 0 for a ray without fine rows.
 *   ADJOINT   g_w_e_j = the sum over the ray's fine rows i in ascending order with j0_i <= j < j1_i of g_loss[r] * c_i (a rounded product,
 *             rounded sums from 0) where w_e_j > 0, and 0 where it is not.  There is no gradient to w_f: mip-NeRF 360 stops it.  No
 *             atomics: the result does not depend on scheduling.
 *   WEIGHTS ADJOINT   for w_i = (1 - exp(-tau_i)) exp(-E_i) and trans = exp(-sum tau) of lab4d_packed_weights:
 *             g_tau_i = g_w_i * exp(-(E_i + tau_i)) - (S - S_i) - g_trans[r] * trans[r], S_i the inclusive PREFIX scan of g_w_k * w_k along
 *             the ray and S its last value.  g_density_i = g_tau_i * deltas_i where TAU counted the row (density_i * deltas_i > 0),
 *             otherwise 0.  A NaN in g_w propagates to the rows of its ray.
 *
 * The library allocates nothing and keeps no pointers; all four calls run on the given stream, read nothing back and are capturable in a
 * hipGraph.  Every kernel: one wave per ray, four rays per block, grid-stride -- the partition of lab4d_packed_composite_forward -- no LDS,
 * no atomics.  Arguments are checked before any launch: 0 <= R, P, Pe, Pf < 2^31, eps >= 0 and finite, non-null where rows exist.
 */
#ifndef LAB4D_PROPOSAL_H
#define LAB4D_PROPOSAL_H

/* density, deltas (P); ray_start, ray_count (R); g_w (P) = dL / dw, g_trans (R) = dL / dtrans or NULL -> g_density (P) in the rows that a
 * ray owns (rows of no ray are left as they are: the caller zero-fills).  tau, E and w are recomputed: two passes over the ray's rows, 64
 * at a time with the carries. */
int lab4d_packed_weights_backward(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P,
                                  const float* g_w, const float* g_trans, float* g_density, void* stream);

/* w_e, t_e, deltas_e (Pe); ray_start_e, ray_count_e (R); dir (R, 3) -> lo_e, hi_e, cdf_e (Pe) = lo, hi, C of every envelope row that a ray
 * owns (rows of no ray are left as they are). */
int lab4d_packed_envelope(const float* w_e, const float* t_e, const float* deltas_e, const int32_t* ray_start_e, const int32_t* ray_count_e, const float* dir,
                          long R, long Pe, float* lo_e, float* hi_e, float* cdf_e, void* stream);

/* lo_e, hi_e, cdf_e (Pe) of the call above with the envelope's (ray_start_e, ray_count_e); the fine list w_f, t_f, deltas_f (Pf) with its
 * (ray_start_f, ray_count_f); dir (R, 3) -> span (Pf, 2) int32 = (j0, j1), coef (Pf) = c (rows of no ray are left as they are), loss (R).
 * Lanes over the ray's fine rows 64 at a time with the carry; two binary searches per fine row. */
int lab4d_packed_proposal_forward(const float* lo_e, const float* hi_e, const float* cdf_e, const int32_t* ray_start_e, const int32_t* ray_count_e, long Pe,
                                  const float* w_f, const float* t_f, const float* deltas_f, const int32_t* ray_start_f, const int32_t* ray_count_f, long Pf,
                                  const float* dir, long R, float eps, int32_t* span, float* coef, float* loss, void* stream);

/* g_loss (R); span, coef of the forward call; w_e (Pe); both (start, count) -> g_w_e (Pe) in the rows that a ray owns (rows of no ray are
 * left as they are).  Lanes over the ray's envelope rows 64 at a time; inside, a loop over the ray's fine rows in ascending order that the
 * whole wave walks together: n_f * ceil(n_e / 64) steps per ray. */
int lab4d_packed_proposal_backward(const float* g_loss, const int32_t* span, const float* coef, const float* w_e, const int32_t* ray_start_e,
                                   const int32_t* ray_count_e, long Pe, const int32_t* ray_start_f, const int32_t* ray_count_f, long Pf, long R, float* g_w_e,
                                   void* stream);

#endif /* LAB4D_PROPOSAL_H */
