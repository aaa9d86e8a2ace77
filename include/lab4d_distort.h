/*
 * lab4d_distort.h -- the distortion loss of a packed sample list, forward and adjoint (included by lab4d_hip.h).
 *
 * Not in the reference (parity unpinned, as for the packed list itself).  The regulariser of Barron et al. 2022 (mip-NeRF 360, eq. 15;
 * nerfacc's `distortion`): per ray, the weights' mutual distances plus their own widths, which pulls a ray's weight into one compact
 * interval.  On a packed list it is a prefix-scan problem per ray, O(n), on the partition of lab4d_packed_composite_forward: nothing of
 * size rays x samples-per-ray and no pair matrix exists.  The per-row arithmetic is lab4d_amd/csrc/distort_math.hpp, shared with the CPU
 * twin tests/host_harness/distort/distort_host.cpp.
 *
 * Rules:
 *   ROWS     ray r owns rows ray_start[r] .. ray_start[r] + ray_count[r] - 1 of a packed list with P rows.  A (start, count) that leaves
 *            [0, P) is cut to it.  Rows that no ray owns are neither read nor written.
 *   WEIGHTS  tau_i = density_i * deltas_i and w_i = (1 - exp(-tau_i)) * exp(-sum_{j<i} tau_j): the COMPOSITE weight of lab4d_packed.h,
 *            formed by the code that lab4d_packed_composite_forward forms it with (the same chunked scan of tau), so that the loss and the
 *            compositor see the same weights on the same rows.
 *   INPUTS   mid_i, the midpoint of row i's interval, ascending within a ray, and width_i >= 0, its width in the units of mid.  Neither
 *            is differentiated.  Gaps between a ray's intervals are legal (empty cells and pruned rows leave them).
 *   LOSS     loss_r = sum_i sum_j w_i w_j |mid_i - mid_j|  +  (1/3) sum_i w_i^2 width_i.   A ray without rows: loss_r = 0.
 *   SHIFT    evaluated on m_i = mid_i - mid_first of the ray (one fp32 subtraction): the loss does not change, and the cancellation at
 *            large mid goes.
 *   O(n)     with the exclusive prefixes W_i = sum_{j<i} w_j and M_i = sum_{j<i} w_j m_j the pair term is 2 sum_i w_i (m_i W_i - M_i).
 *   ADJOINT  with the ray totals W, M and the inclusive prefixes W_i + w_i, M_i + w_i m_i:
 *              g_w_i   = 2 [ (m_i W_i - M_i) + ((M - M_i - w_i m_i) - m_i (W - W_i - w_i)) ] + (2/3) w_i width_i
 *              g_tau_i = g_w_i exp(-sum_{j<=i} tau_j) - S_i,     S_i = sum_{j>i} g_w_j w_j
 *              g_density_i = g_loss_r g_tau_i deltas_i,          g_deltas_i = g_loss_r g_tau_i density_i
 *            The loss is homogeneous of degree 2 in w: sum_j g_w_j w_j = 2 loss_r, so S_i = 2 loss_r - (the inclusive prefix of g_w w).
 *            The adjoint is two FORWARD sweeps over the ray (totals and loss, then the gradients): no suffix scan, no scratch.
 *   SUMS     fp32.  The prefixes of tau, w, w m and g_w w run in chunks of 64 rows with a carry, the loss as per-lane partial sums that
 *            meet at the end of the ray; the order differs from a serial sum, so the results are held to the float64 definition within
 *            the project's fp32 bar, not word for word.
 *
 * The library allocates nothing and keeps no pointers; both calls run on the given stream, read nothing back and are capturable in a
 * hipGraph.  Arguments are checked before any launch: 0 <= R, P < 2^31, non-NULL required pointers.
 */
#ifndef LAB4D_DISTORT_H
#define LAB4D_DISTORT_H

/* density, deltas, mid, width (P); ray_start, ray_count (R) -> loss (R), written for every ray.  One wave per ray, lanes over the ray's
 * consecutive rows 64 at a time with the carries. */
int lab4d_packed_distortion_forward(const float* density, const float* deltas, const float* mid, const float* width, const int32_t* ray_start,
                                    const int32_t* ray_count, long R, long P, float* loss, void* stream);

/* The same inputs and the cotangent g_loss (R) -> g_density (P) or NULL, g_deltas (P) or NULL.  Rows of no ray are left as they are: the
 * caller zeroes them.  With both NULL the call returns without a launch. */
int lab4d_packed_distortion_backward(const float* density, const float* deltas, const float* mid, const float* width, const int32_t* ray_start,
                                     const int32_t* ray_count, long R, long P, const float* g_loss, float* g_density, float* g_deltas, void* stream);

#endif /* LAB4D_DISTORT_H */
