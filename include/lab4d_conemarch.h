/*
 * lab4d_conemarch.h -- cascaded occupancy grids and cone-stepped packed marching for the hash field (included by lab4d_hip.h).
 *
 * Not in the reference (nnutils/nerf.py:98 is a TODO; parity unpinned, as for the hash field itself): the march of lab4d_packed.h walks one
 * G^3 bit grid over one box at one fixed step, which fits an object box and not a scene box many times as wide.  Here the step grows with
 * the distance, dt = clamp(t * cone_angle, dt_min, dt_max), and a cascade of K occupancy grids, each twice the extent of the one before
 * around the same centre, is looked up per sample at the level that fits the sample's position and its step (Mueller et al. 2022,
 * appendix E).  The marcher emits the packed layout of lab4d_packed.h, so every consumer of a packed list (composite, prune, distortion,
 * weights / resample, merge, render_weights / proposal_loss) takes its output unchanged.  The arithmetic is
 * lab4d_amd/csrc/conemarch_math.hpp over occgrid_math.hpp and ray_math.hpp, shared with the CPU twin
 * tests/host_harness/conemarch/conemarch_host.cpp, which the kernels equal word for word.
 *
 * Rules:
 *   CASCADE  K levels, 1 <= K <= 8.  One G for all levels, 2 <= G <= 256; G must be even when K > 1.  aabbs (K, 6) fp32 on the device,
 *            level c = {lo xyz, hi xyz}; the kernels take the boxes as given (the Python container builds level c as centre +- half
 *            extent * 2^c of the base box, in float64, rounded once to fp32).  bits (K, n_words(G)), each level in the layout of
 *            lab4d_occgrid.h.
 *   EDGE     edge_c = the minimum over the three axes of (hi - lo) / G, the correctly rounded fp32 quotient.
 *   LEVEL    of a point p with a step of world length delta:  c_pos = the smallest c for which p has a cell in box c (GRID of
 *            lab4d_occgrid.h); none: the point is not kept.  c_step = the smallest c with delta <= edge_c; none: c_step = K - 1.
 *            level = max(c_pos, c_step).  The point is kept iff the MASK of lab4d_occgrid.h is set for p in box `level` with that level's bits.
 *   STEPS    ray o + t d, t in [t0, t1], d of any length.  The CLIP of the rays (csrc/ray_math.hpp) against box K - 1 gives [t_in, t_out]
 *            within [t0, t1]; a miss gives count 0, so does a non-finite o, d, t0 or t1, and so does t0 > t1.  a_0 = t_in;
 *            s_k = min(max(a_k * cone, dt_min), dt_max);  t_k = a_k + 0.5 * s_k;  a_{k+1} = a_k + s_k  -- every product and sum rounded to
 *            fp32 on its own.  Candidate k exists while k < k_max and t_k <= t_out; the walk ends at the first k that fails.  The
 *            recurrence is the definition: it accumulates by nature and is deterministic because every operation is rounded on its own.
 *            p_k = o + t_k d (product and sum rounded on their own), delta_k = s_k * |d|.  An implementation may skip lookups through
 *            known-empty space; it must not change the candidate sequence or the kept set.
 *   PER ROW  t = t_k, steps = s_k, deltas = delta_k, xyz = p_k, dirs = d / |d| exactly as lab4d_packed_march_write writes it, ray_idx and
 *            level per row.
 *   LAYOUT   the LAYOUT of lab4d_packed.h, word for word: ray order, ascending k within a ray; count, then the caller's exclusive scan,
 *            then write; a STATIC cap; ray_count_out clamped; total untruncated; overflow = total > cap.  Rows in [min(total, cap), cap)
 *            are parked with the park point of box K - 1 (hi + (hi - lo)): dirs = (0, 0, 1), t = steps = deltas = 0,
 *            ray_idx = level = -1.  No atomics.
 *
 * Every call runs on the given stream, reads nothing back, allocates nothing and is capturable in a hipGraph.  Arguments are checked before
 * any launch: cone finite and >= 0; 0 < dt_min <= dt_max, both finite; k_max >= 1; R * k_max < 2^31; 0 <= cap < 2^31; K and G as in CASCADE.
 */
#ifndef LAB4D_CONEMARCH_H
#define LAB4D_CONEMARCH_H

/* LEVEL per point: xyz (S, 3), delta (S) or NULL (= 0 for every point), aabbs (K, 6), bits (K, n_words(G)) -> mask (S) uint8,
 * level (S) int32 or NULL: max(c_pos, c_step), -1 where the point has no cell in any box.  One lane per point. */
int lab4d_occgrid_cascade_mask(const float* xyz, const float* delta, const float* aabbs, const uint32_t* bits, int K, int G, long S,
                               uint8_t* mask, int32_t* level, void* stream);

/* origin, dir (R, 3), t_range (R, 2) = {t0, t1}, aabbs, bits -> ray_count (R) int32.  One lane per ray. */
int lab4d_packed_march_cone_count(const float* origin, const float* dir, const float* t_range, const float* aabbs, const uint32_t* bits,
                                  int K, int G, long R, float cone, float dt_min, float dt_max, int k_max, int32_t* ray_count, void* stream);

/* The same rays again, with ray_start (R) = the exclusive prefix sum of lab4d_packed_march_cone_count's ray_count, and the capacity ->
 * t, steps, deltas (cap), xyz, dirs (cap, 3), ray_idx, level (cap) int32, ray_count_out (R) int32 (clamped), total (1) int32,
 * overflow (1) uint8.  One lane per ray writes the ray's rows; the rows behind min(total, cap) are parked by a second launch. */
int lab4d_packed_march_cone_write(const float* origin, const float* dir, const float* t_range, const float* aabbs, const uint32_t* bits,
                                  int K, int G, long R, float cone, float dt_min, float dt_max, int k_max, const int32_t* ray_start,
                                  long cap, float* t, float* steps, float* deltas, float* xyz, float* dirs, int32_t* ray_idx,
                                  int32_t* level, int32_t* ray_count_out, int32_t* total, uint8_t* overflow, void* stream);

#endif /* LAB4D_CONEMARCH_H */
