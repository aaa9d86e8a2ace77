/*
 * lab4d_prune.h -- pruning of a packed sample list by transmittance and opacity (included by lab4d_hip.h).
 *
 * Not in the reference (parity unpinned, as for the packed list itself).  lab4d_packed.h removes the samples in empty space; what remains
 * are the samples BEHIND the surface: once a ray's transmittance has fallen to nothing, every further kept row still pays the encoding, both
 * nets and the table atomics, forward and backward.  The two-pass form of Mueller et al. 2022 (section 5.4 / appendix E) and of nerfacc:
 * march once, take the density of the kept rows without gradients, PRUNE the packed list with the two calls below, and run the
 * differentiable field on the survivors only.  No kernel loops over rounds, no ray state lives between launches, and the layout of the
 * result is a pure function of the inputs, like the march's.  The arithmetic is lab4d_amd/csrc/prune_math.hpp, shared with the CPU twin
 * tests/host_harness/prune/prune_host.cpp, to which both kernels are held word for word.
 *
 * Rules:
 *   ROWS     ray r owns rows ray_start[r] .. ray_start[r] + ray_count[r] - 1 of a packed list with P rows.  A (start, count) that leaves
 *            [0, P) is cut to it.
 *   TAU      tau_i = density_i * deltas_i (one rounded fp32 product).  A tau that is NaN or not > 0 counts as 0 (the occupancy grid's rule
 *            for densities).
 *   PREFIX   E_i, the exclusive prefix sum of tau along the ray, in fp32 and in one stated order: rows in chunks of 64 from the ray's
 *            first row; inside a chunk the doubling scan  for o = 1, 2, 4 .. 32: v[l] += v[l - o] for l >= o  (plain fp32 adds, dead lanes
 *            hold 0); then + carry, the inclusive value of the previous chunk's lane 63 (0 for the first chunk).  E_i is the inclusive value
 *            of the lane before, carry itself for lane 0.  This is the scan of lab4d_packed_composite_forward.
 *   STOP     j* = the first row of the ray with E_j > tau_stop -- over the chunks in order, the lowest lane inside a chunk, so the stop
 *            is monotone by construction even where an fp32 prefix dips by an ulp.  Every row >= j* is dropped.  tau_stop = +inf never
 *            stops.
 *   OPACITY  a row before the stop is kept iff tau_i >= tau_min; tau_min = 0 keeps all of them.  Dropped rows still count in the prefix
 *            of the rows behind them: transmittance is a property of the ray, not of the kept set.
 *   NO EXP   the kernels compare in the tau domain.  The caller converts in double precision and rounds to fp32 once:
 *            tau_stop = -log(early_stop_eps) (+inf for 0), tau_min = -log1p(-alpha_thre).
 *   LAYOUT   the march's contract again.  Survivors in ray order, ascending row within a ray.  new_count[r] = survivors of ray r,
 *            new_start = its exclusive prefix sum (the caller's scan between the two calls), total = the sum.  The capacity cap is STATIC:
 *            rows >= cap are not written, the emitted new_count_out[r] = clamp(cap - new_start[r], 0, new_count[r]), overflow = total > cap,
 *            total is the untruncated sum.  Rows in [min(total, cap), cap) are parked exactly as the march parks them: xyz = hi + (hi - lo)
 *            of the box aabb, dirs = (0, 0, 1), ray_idx = -1, t = deltas = 0, and src_row = -1.  A surviving row copies t, deltas, xyz and
 *            dirs bit for bit from its source row; ray_idx is the owning ray; src_row is the source row's index, so that a caller can gather
 *            what it already computed per row.  No atomics: the result does not depend on scheduling.
 *
 * The library allocates nothing and keeps no pointers; both calls run on the given stream, read nothing back and are capturable in a
 * hipGraph.  Arguments are checked before any launch: 0 <= R, P < 2^31, 0 <= cap < 2^31, tau_stop >= 0 or +inf and not NaN, tau_min >= 0
 * and finite.
 */
#ifndef LAB4D_PRUNE_H
#define LAB4D_PRUNE_H

/* density, deltas (P); ray_start, ray_count (R) -> keep (P) uint8: 1 for a survivor, 0 for every other row that a ray owns (rows of no
 * ray are left as they are: the caller zero-fills), new_count (R) int32.  One wave per ray, lanes over the ray's consecutive rows 64 at a
 * time with the carry; a wave stops scanning at the chunk that holds the stop and only clears keep behind it. */
int lab4d_packed_prune_count(const float* density, const float* deltas, const int32_t* ray_start, const int32_t* ray_count, long R, long P,
                             float tau_stop, float tau_min, uint8_t* keep, int32_t* new_count, void* stream);

/* keep (P) of the call above, the same (ray_start, ray_count), new_start (R) = the exclusive prefix sum of new_count, the capacity, the
 * box aabb (6) of the park point, and the source list t, deltas (P), xyz, dirs (P, 3) -> t_out, deltas_out (cap), xyz_out, dirs_out
 * (cap, 3), ray_idx_out, src_row_out (cap) int32, new_count_out (R) int32 (clamped), total (1) int32, overflow (1) uint8.  The same
 * partition; a survivor's place inside its chunk comes from a ballot and a popcount, so a wave's survivors leave as consecutive rows.
 * The rows behind min(total, cap) are parked by a second launch.  (aabb: the source list does not carry its box.) */
int lab4d_packed_prune_write(const uint8_t* keep, const int32_t* ray_start, const int32_t* ray_count, const int32_t* new_start, long R, long P,
                             long cap, const float* aabb, const float* t, const float* deltas, const float* xyz, const float* dirs, float* t_out,
                             float* deltas_out, float* xyz_out, float* dirs_out, int32_t* ray_idx_out, int32_t* src_row_out,
                             int32_t* new_count_out, int32_t* total, uint8_t* overflow, void* stream);

#endif /* LAB4D_PRUNE_H */
