/*
 * lab4d_hashtrace.h -- sphere tracing of the hash field's SDF to one surface hit per ray (included by lab4d_hip.h).
 *
 * The hash field's geometry output is a signed distance (lab4d_hashsdf.h).  Instead of marching a lattice through the occupied cells
 * (lab4d_packed.h) a ray takes steps of the size the distance allows (Hart 1996) until |sdf| <= eps, then needs one colour and one normal
 * evaluation at the hit: a preview / eval path, a depth or normal map without a mesh, surface points for the eikonal term, a per-ray near
 * bound.  Not in the reference (no hash field, no tracer): the rules are this repository's own, parity is unpinned, the truth of the tests
 * is float64 over oracle/hashgrid_oracle.py.  The arithmetic is lab4d_amd/csrc/hashtrace_math.hpp over hashsdf_math.hpp, occgrid_math.hpp
 * and packed_math.hpp, shared with the CPU twin tests/host_harness/hashtrace/hashtrace_host.cpp.  fp32 throughout.
 *
 * Rules (ray o + t * d, t in [t0, t1], d of any length, len = |d| rounded as in lab4d_packed.h; aabb = {lo, hi}):
 *   STATUS    0 MISS, 1 CONVERGED, 2 BRACKETED, 3 STARTS_INSIDE, 4 OUT_OF_STEPS.
 *   REJECT    a non-finite o, d, t0 or t1, t0 > t1, len == 0 or a box without extent: status 0, t_hit = t0, n_eval = 0, sdf_hit = 0.
 *   CLIP      [t0, t1] is cut to the box with the slab test of lab4d_occgrid.h (SPAN) in x01 space: a parallel axis is always or never
 *             satisfied, no inf or NaN arithmetic occurs.  An empty clip is handled like a rejected ray; otherwise t_enter <= t_exit.
 *   EVAL      p = o + t * d (product and sum rounded on their own); x01 = (p - lo) / (hi - lo) clamped to [0, 1] per axis, so that the
 *             constant sdf outside the box is never traced; s = the sdf of lab4d_hashsdf.h (FORWARD) at x01.
 *   LOOP      t = t_enter, evaluate s.  The first s <= 0: STARTS_INSIDE, t_hit = t_enter.  |s| <= eps: CONVERGED, t_hit = t.  s < -eps
 *             after a positive previous value: [t_prev, t] is bisected at most n_bisect times, one evaluation at the midpoint each, the end
 *             with the positive value stays the lower one, stopped early at |s_mid| <= eps: BRACKETED, t_hit = the last midpoint evaluated
 *             (n_bisect == 0: t).  Otherwise step: t == t_exit already: MISS, t_hit = t_exit; t_next = t + max(step_scale * s, min_step)
 *             / len, cut to t_exit (the last evaluation sits on the exit face); t_next <= t after rounding: OUT_OF_STEPS.  After max_steps
 *             evaluations outside bisections: OUT_OF_STEPS, t_hit = the last t.
 *   OUTPUTS   t_hit, status, n_eval, sdf_hit are written for every ray; sdf_hit is the sdf at t_hit; n_eval <= max_steps + n_bisect; t never
 *             runs backwards outside a bisection; t_enter <= t_hit <= t_exit for a ray that enters the box.
 *
 * One lane per ray, 256 per workgroup, the net's 8.5 KB in LDS; a lane leaves the loop when its ray ends.  No atomics, no read-back, no
 * allocation: capturable in a hipGraph.  Arguments are checked before any launch: 0 <= R < 2^31 (R == 0 is a successful no-op),
 * L * F == 32, L <= 32, F <= 8 (F is 1, 2, 4 or 8), 4 <= log2_T <= 24, eps > 0 and finite, 0 < step_scale <= 1, min_step > 0 and finite,
 * 1 <= max_steps <= 1024, 0 <= n_bisect <= 32, every pointer non-NULL (at R == 0 the per-ray arrays are empty and may be NULL).
 */
#ifndef LAB4D_HASHTRACE_H
#define LAB4D_HASHTRACE_H

/* origin, dir (R,3), t_range (R,2) = {t0, t1}, aabb (6), table (L, 2^log2_T, F), res (L) int32, W1 (64,32), b1 (64), w2 (64), b2 (1)
 * -> t_hit (R), status (R) int32, n_eval (R) int32, sdf_hit (R). */
int lab4d_hashsdf_trace(const float* origin, const float* dir, const float* t_range, const float* aabb, long R, const float* table,
                        const int32_t* res, int L, int log2_T, int F, const float* W1, const float* b1, const float* w2, const float* b2,
                        float eps, float step_scale, float min_step, int max_steps, int n_bisect, float* t_hit, int32_t* status,
                        int32_t* n_eval, float* sdf_hit, void* stream);

#endif /* LAB4D_HASHTRACE_H */
