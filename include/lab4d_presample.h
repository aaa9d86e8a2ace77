/*
 * lab4d_presample.h -- importance resampling of a packed sample list per ray: the compositing weights of the list, and its inverse-CDF
 * resampling into a new packed list of n_imp rows per ray (included by lab4d_hip.h).
 *
 * The reference's renderer is coarse-to-fine: NeRF.importance_sampling (nnutils/nerf.py:686-738) takes the density of a coarse pass without
 * gradients, turns it into weights (compute_weights, utils/render_utils.py:99-131) and draws the fine depths by inverse CDF
 * (render_utils.sample_pdf, utils/render_utils.py:187-233).  lab4d_sample_pdf does that for the dense (M, N, D) layout; the three calls below
 * do it for a packed list (lab4d_packed.h, lab4d_prune.h, lab4d_pmerge.h), whose rays have their own lengths.  The reference has no packed
 * lists, so parity is unpinned by nature and the rules are this repository's own.  The result is again a packed list with a per-ray
 * (start, count), sorted in t: lab4d_packed_composite_*, lab4d_packed_distortion_* and lab4d_packed_merge_* take it as it is.  The arithmetic
 * is lab4d_amd/csrc/presample_math.hpp, shared with the CPU twin tests/host_harness/presample/presample_host.cpp, to which both resample kernels
 * are held word for word (they call no exp: the weights come in).
 *
 * Rules:
 *   ROWS     ray r owns rows ray_start[r] .. ray_start[r] + ray_count[r] - 1 of a packed list with P rows.  A (start, count) that leaves
 *            [0, P) is cut to it (rows_of of prune_math.hpp).  n is the cut count.
 *   WEIGHTS  tau_i = density_i * deltas_i, NaN or not > 0 counting as 0 (TAU of lab4d_prune.h).  E_i = the exclusive prefix of tau along the
 *            ray in the PREFIX order of lab4d_prune.h: chunks of 64, doubling scan, carry.  w_i = (1 - exp(-tau_i)) * exp(-E_i), the
 *            reference's compute_weights; trans[r] = exp(-(the inclusive value of the ray's last row)), 1 for a ray without rows.
 *   MASS     m_i = max(w_i, 0) + eps (one rounded fp32 sum), a NaN weight counting as 0.  C_i is the inclusive prefix of m along the ray in
 *            the same PREFIX order, E_i the exclusive one (C of the row before, 0 for the first), W = C of the ray's last row.
 *   COUNT    new_count[r] = n_imp if the ray owns at least one row and W > 0, otherwise 0.  new_start is its exclusive prefix sum: the
 *            caller's scan between the two calls, as for the march, the prune and the merge.
 *   QUERY    u_k = (k + 0.5) / n_imp (one rounded fp32 quotient) when u == NULL, otherwise the caller's u[r * n_imp + k] clamped to [0, 1]
 *            (NaN -> 0); that input is meant to be non-decreasing per ray.  q_k = u_k * W (one rounded product).
 *   ROW      i_k = min(#{i : C_i <= q_k}, n - 1) by one binary search (count_before of pmerge_math.hpp).  Where C is monotone that is the
 *            first row with C_i > q_k; where an fp32 prefix dips by an ulp the search still returns a row of the ray, the same one on both
 *            sides, after at most ceil(log2(n + 1)) steps whatever it reads.
 *   PLACE    f = clamp((q_k - E_i) / m_i, 0, 1) (0 for 0 / 0).  The row's interval in t is centred on t_i and deltas_i / |dir_r| wide,
 *            |dir| as the march forms it for deltas (the root of the three rounded squares added x, y, z); the width is 0 for |dir| = 0.
 *            t'_k = t_i + (f - 0.5) * width, every operation rounded on its own.
 *   ORDER    the emitted t_k is the running maximum of t' over k' <= k within the ray.  The list is therefore non-decreasing in t within
 *            every ray whatever the input: the precondition of lab4d_packed_merge_write.
 *   SPAN     deltas_k = min(deltas_i, (deltas_i * W) / (n_imp * m_i)): the length along the ray that carries 1 / n_imp of the mass, never
 *            more than the source row's own.  With stratified u the new rows inside a source row sum to about that row's length, so the
 *            list is a quadrature for lab4d_packed_composite_forward on its own.
 *   PER ROW  xyz = o + t_k * d (product and sum rounded on their own), dirs = d / |d| exactly as the march writes it, ray_idx = r, src_row =
 *            the global index of source row i_k.
 *   LAYOUT   the march's contract, word for word.  The capacity cap is STATIC: rows >= cap are not written, the emitted new_count_out[r] =
 *            clamp(cap - new_start[r], 0, new_count[r]), total is the untruncated sum, overflow = total > cap.  Rows in [min(total, cap),
 *            cap) are parked as the march parks them: xyz = hi + (hi - lo) of the box aabb, dirs = (0, 0, 1), t = deltas = 0, ray_idx =
 *            src_row = -1.  No atomics: the result does not depend on scheduling.
 *
 * The library allocates nothing and keeps no pointers; all three calls run on the given stream, read nothing back and are capturable in a
 * hipGraph.  No buffer of size rays x samples exists other than the outputs; rays of any length and any n_imp are supported.  Arguments
 * are checked before any launch: 0 <= R, P, cap < 2^31, 1 <= n_imp, R * n_imp < 2^31, eps >= 0 and finite.
 */
#ifndef LAB4D_PRESAMPLE_H
#define LAB4D_PRESAMPLE_H

/* density, deltas (P); ray_start, ray_count (R) -> w (P), the compositing weight of every row that a ray owns (rows of no ray are left as
 * they are: the caller zero-fills), and trans (R) or NULL.  One wave per ray, lanes over the ray's consecutive rows 64 at a time with the
 * carry: the partition and the scan of lab4d_packed_composite_forward. */
int lab4d_packed_weights(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P, float* w,
                         float* trans, void* stream);

/* weights (P); ray_start, ray_count (R) -> cdf (P) = C_i (rows of no ray are left as they are), mass (R) = W, new_count (R) int32.  The
 * same partition. */
int lab4d_packed_resample_count(const float* weights, const int32_t* ray_start, const int32_t* ray_count, long R, long P, int n_imp, float eps,
                                float* cdf, float* mass, int32_t* new_count, void* stream);

/* weights, cdf (P) and mass (R) of the call above with the same n_imp and eps, the source list t, deltas (P) and its (ray_start, ray_count),
 * new_start (R) = the exclusive prefix sum of new_count, the rays origin, dir (R, 3), u (R, n_imp) or NULL, the capacity and the box aabb
 * (6) of the park point -> t_out, deltas_out (cap), xyz_out, dirs_out (cap, 3), ray_idx_out, src_row_out (cap) int32, new_count_out (R)
 * int32 (clamped), total (1) int32, overflow (1) uint8.  One wave per ray, lanes over the ray's n_imp samples 64 at a time with the carry
 * of the running maximum; one binary search over the ray's cdf per sample.  The rows behind min(total, cap) are parked by a second launch. */
int lab4d_packed_resample_write(const float* weights, const float* cdf, const float* mass, const float* t, const float* deltas, const int32_t* ray_start,
                                const int32_t* ray_count, const int32_t* new_start, long R, long P, const float* origin, const float* dir, const float* u,
                                int n_imp, float eps, long cap, const float* aabb, float* t_out, float* deltas_out, float* xyz_out, float* dirs_out,
                                int32_t* ray_idx_out, int32_t* src_row_out, int32_t* new_count_out, int32_t* total, uint8_t* overflow, void* stream);

#endif /* LAB4D_PRESAMPLE_H */
