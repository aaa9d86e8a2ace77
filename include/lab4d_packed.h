/*
 * lab4d_packed.h -- packed ray marching and ragged compositing for the hash field (included by lab4d_hip.h).
 *
 * Not in the reference (nnutils/nerf.py:98 is a TODO; parity unpinned, as for the hash field itself): a ray is marched at a fixed step
 * through the occupied cells of the occupancy bit grid (lab4d_occgrid.h) only, the kept samples of all rays form one packed list with a
 * per-ray (start, count), and the list is composited directly (Mueller et al. 2022, section 5.4 / appendix E).  Nothing of size
 * rays x samples-per-ray exists.  The arithmetic is lab4d_amd/csrc/packed_math.hpp over lab4d_amd/csrc/occgrid_math.hpp, shared with the
 * CPU twin tests/host_harness/packed_host.cpp; the march kernels equal the twin word for word, the compositing kernels equal the
 * reference's compute_weights + integrate (utils/render_utils.py:99-160) on every ray alone to fp32 rounding.
 *
 * Rules:
 *   MARCH      ray o + t * d, t in [t0, t1]; d need not have unit length, t and the step dt > 0 are in the caller's depth units.
 *              Candidates sit on the ray's own lattice t_k = t0 + (k + 0.5) * dt (product and sum rounded on their own, formed from k every
 *              time), 0 <= k < K, K = min(k_max, number of k with t_k <= t1), k_max >= 1.  The SPAN of lab4d_occgrid.h is taken first: a ray
 *              that misses keeps nothing, otherwise only the k with t_first <= t_k <= t_last are looked at; candidate k is kept iff the MASK
 *              of lab4d_occgrid.h is set for p_k = o + t_k * d (again rounded on their own).  The span only prunes the loop: the per-point
 *              bit decides what is kept.  A non-finite o, d, t0 or t1, or t0 > t1: count 0.  Per kept sample: t = t_k, xyz = p_k,
 *              dirs = d / |d|, deltas = dt * |d| (the same for every sample of a ray), ray_idx = the ray.
 *   LAYOUT     kept samples in ray order, ascending k within a ray.  ray_count[r] = kept samples of ray r, ray_start = exclusive prefix sum
 *              of ray_count (the caller's scan between the two march calls), total = sum of ray_count.  The capacity cap is STATIC: rows
 *              >= cap are not written, the emitted ray_count_out[r] = clamp(cap - ray_start[r], 0, ray_count[r]), overflow = total > cap,
 *              total is the untruncated sum.  Rows in [min(total, cap), cap) are parked: xyz = hi + (hi - lo) (outside the box),
 *              dirs = (0, 0, 1), ray_idx = -1, t = 0, deltas = 0.  The layout does not depend on scheduling.
 *   COMPOSITE  ray r owns rows ray_start[r] .. ray_start[r] + ray_count[r] - 1 of the packed (P, .) arrays:  tau_i = density_i * deltas_i,
 *              T_i = exp(-sum_{j<=i} tau_j),  w_i = (1 - exp(-tau_i)) * exp(-sum_{j<i} tau_j),  mask = sum w.  Field modes are those of
 *              lab4d_composite_forward: 0 = sum w / (mask + 1e-6) * v, 1 = the same with detached weights, 2 = plain mean over the ray's
 *              samples and channels (one output).  A ray without samples: mask = 0 and every output 0, mode 2 included.  Rows that no
 *              ray owns are neither read nor written.  A (start, count) that leaves [0, P) is cut to it.
 *
 * The library allocates nothing and keeps no pointers; every call runs on the given stream, reads nothing back and is capturable in a
 * hipGraph.  Arguments are checked before any launch: dt finite and > 0, k_max >= 1, R * k_max < 2^31, 0 <= cap < 2^31, 2 <= G <= 256.
 */
#ifndef LAB4D_PACKED_H
#define LAB4D_PACKED_H

/* origin, dir (R, 3), t_range (R, 2) = {t0, t1}, aabb (6), bits (the grid's words) -> ray_count (R) int32.  One lane per ray. */
int lab4d_packed_march_count(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G,
                             long R, float dt, int k_max, int32_t* ray_count, void* stream);

/* The same rays again, with ray_start (R) = the exclusive prefix sum of lab4d_packed_march_count's ray_count, and the capacity ->
 * t (cap), deltas (cap), xyz (cap, 3), dirs (cap, 3), ray_idx (cap) int32, ray_count_out (R) int32 (clamped), total (1) int32,
 * overflow (1) uint8.  One lane per ray writes the ray's rows; the rows behind min(total, cap) are parked by a second launch. */
int lab4d_packed_march_write(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G,
                             long R, float dt, int k_max, const int32_t* ray_start, long cap, float* t, float* deltas, float* xyz,
                             float* dirs, int32_t* ray_idx, int32_t* ray_count_out, int32_t* total, uint8_t* overflow, void* stream);

/* density, deltas (P); fields[i] (P, channels[i]); ray_start, ray_count (R) -> weights, transmit (P) (each may be NULL; rows of no ray
 * are left as they are), mask (R), out (R, sum channels) in field order (a mode-2 field has one output).  One wave per ray, lanes over
 * the ray's consecutive rows, 64 at a time with a carry.  sum channels <= 64. */
int lab4d_packed_composite_forward(const float* density, const float* deltas, const lab4d_field_list* fl, const int32_t* ray_start,
                                   const int32_t* ray_count, long R, long P, float* weights, float* transmit, float* mask, float* out,
                                   void* stream);

/* Adjoint of the above.  g_mask (R), g_out (R, sum channels): each may be NULL (= zero).  Outputs, each may be NULL: g_density,
 * g_deltas (P), g_fields[i] (P, channels[i]); rows of no ray are left as they are (the caller zeroes them).  A mode-1 field gives no
 * gradient to the weights. */
int lab4d_packed_composite_backward(const float* density, const float* deltas, const lab4d_field_list* fl, const int32_t* ray_start,
                                    const int32_t* ray_count, long R, long P, const float* g_mask, const float* g_out, float* g_density,
                                    float* g_deltas, const lab4d_field_grads* g_fields, void* stream);

#endif /* LAB4D_PACKED_H */
