/*
 * lab4d_pmerge.h -- merge of two packed sample lists per ray by depth, and the gather of per-row values through it (included by lab4d_hip.h).
 *
 * The reference renders a foreground field in front of a background: MultiFields.compose_fields (nnutils/multifields.py:339-398)
 * concatenates the samples of both fields along the depth axis, z-sorts them per ray with an argsort and gathers every per-sample key,
 * deltas included, through that permutation.  lab4d_compose_order / lab4d_compose_gather do that for the dense (M, N, D) layout; the three
 * calls below do it for two packed lists (lab4d_packed.h, lab4d_prune.h), whose rays have their own lengths.  The result is again a packed
 * list with a per-ray (start, count): lab4d_packed_composite_* and lab4d_packed_distortion_* take it as it is.  The arithmetic is
 * lab4d_amd/csrc/pmerge_math.hpp, shared with the CPU twin tests/host_harness/pmerge/pmerge_host.cpp, to which the kernels are held word
 * for word.
 *
 * Rules:
 *   ROWS     list A has Pa rows and list B has Pb rows, Pa + Pb < 2^31.  Ray r owns rows start[r] .. start[r] + count[r] - 1 of each list
 *            (rows_of of prune_math.hpp); a (start, count) that leaves [0, P) is cut to it.  na and nb are the cut counts.
 *   ORDER    both lists must be non-decreasing in t within every ray (the march and the prune emit them that way) and free of NaN, and
 *            both must measure t in the same units along the same ray.  That is the caller's business: the two fields may live in
 *            different frames, which is why a merged list carries no xyz / dirs.  The merged order of ray r is the stable argsort of
 *            [t_a | t_b]: a tie between the lists goes to A, the order inside a list is kept (lab4d_compose_order's rule).  As ranks, so
 *            that every input row finds its place on its own:
 *              A's i-th row of the ray goes to  i + #{j : t_b[j] <  t_a[i]},
 *              B's j-th row of the ray goes to  j + #{i : t_a[i] <= t_b[j]}.
 *            Each count is one binary search (count_before of pmerge_math.hpp).  Comparisons are plain fp32 < and <=: -0.0 ties with 0.0.
 *            For input that breaks the precondition the result is unspecified, with two guarantees: every write stays inside the ray's
 *            na + nb merged rows, and the call terminates (a search takes at most ceil(log2(n + 1)) steps whatever it reads).
 *   LAYOUT   the march's and the prune's.  count[r] = na + nb, start = its exclusive prefix sum (the caller's scan between the two calls),
 *            total = the sum, untruncated.  The capacity cap is STATIC: rows >= cap are not written, ray_count_out[r] =
 *            clamp(cap - start[r], 0, count[r]), overflow = total > cap.  Rows in [min(total, cap), cap) are parked with t = 0,
 *            deltas = 0, ray_idx = -1, src = -1.  No atomics: the layout does not depend on scheduling.
 *   PER ROW  t and deltas are copied bit for bit from the source row (the reference gathers deltas, it does not recompute them);
 *            ray_idx = the ray; src = the source row in the concatenation: i for A's row i, Pa + i for B's row i.  The inverse is
 *            pos_a (Pa) and pos_b (Pb): the merged row that an input row went to, -1 for a row that no ray owns or that fell behind cap.
 *   GATHER   out[j, :] = 0 if idx[j] < 0, a[idx[j], :] if idx[j] < Pa, b[idx[j] - Pa, :] if idx[j] < Pa + Pb, and 0 behind that (no row is
 *            read outside the two parts).  A NULL part reads as zeros: a key that only one field produces (multifields.py:381-387).
 *            Forward: idx = src.  Adjoint of part A: the same call with a = g_out, Pa := the merged list's rows, b = NULL, idx = pos_a;
 *            part B likewise with pos_b.  Every value is a copy, so the adjoint is the exact transpose.
 *
 * The library allocates nothing and keeps no pointers; all three calls run on the given stream, read nothing back and are capturable in a
 * hipGraph.  Arguments are checked before any launch: 0 <= R < 2^31, 0 <= Pa, Pb, Pa + Pb < 2^31, 0 <= cap < 2^31, 0 <= n < 2^31,
 * 1 <= C <= 64.
 */
#ifndef LAB4D_PMERGE_H
#define LAB4D_PMERGE_H

/* start_a, count_a, start_b, count_b (R) int32 -> ray_count (R) int32 = na + nb.  One lane per ray. */
int lab4d_packed_merge_count(const int32_t* start_a, const int32_t* count_a, long Pa, const int32_t* start_b, const int32_t* count_b, long Pb, long R,
                             int32_t* ray_count, void* stream);

/* t_a, deltas_a (Pa), t_b, deltas_b (Pb), both (start, count), ray_start (R) = the exclusive prefix sum of the counts of the call above, the
 * capacity -> t, deltas (cap), ray_idx, src (cap) int32, pos_a (Pa), pos_b (Pb) int32, ray_count_out (R) int32 (clamped), total (1) int32,
 * overflow (1) uint8.  Three launches: pos_a and pos_b are filled with -1, so that ALL of them is written; then one wave per ray, lanes
 * over the ray's A rows and then its B rows, one binary search over the other list per row; then the rows behind min(total, cap) are
 * parked, as the march parks them. */
int lab4d_packed_merge_write(const float* t_a, const float* deltas_a, const int32_t* start_a, const int32_t* count_a, long Pa, const float* t_b,
                             const float* deltas_b, const int32_t* start_b, const int32_t* count_b, long Pb, long R, const int32_t* ray_start, long cap,
                             float* t, float* deltas, int32_t* ray_idx, int32_t* src, int32_t* pos_a, int32_t* pos_b, int32_t* ray_count_out,
                             int32_t* total, uint8_t* overflow, void* stream);

/* a (Pa, C) or NULL, b (Pb, C) or NULL, idx (n) int32 -> out (n, C) by the GATHER rule.  Lanes over the n * C values of out. */
int lab4d_packed_merge_gather(const float* a, long Pa, const float* b, long Pb, const int32_t* idx, long n, int C, float* out, void* stream);

#endif /* LAB4D_PMERGE_H */
