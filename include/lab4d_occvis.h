/*
 * lab4d_occvis.h -- camera-visibility culling of the occupancy grids of the hash field (included by lab4d_hip.h).
 *
 * Not in the reference (parity unpinned, as for the occupancy grid itself).  Every occupancy bit of lab4d_occgrid.h / lab4d_conemarch.h comes
 * from the field's own density at the cell centres; in a scene box many times as wide as the object most cells are never crossed by a
 * training ray, their hash entries keep their initialisation and their density is noise no loss ever touched.  Instant-NGP
 * (mark_untrained_density_grid) and nerfacc (mark_invisible_cells) clear the cells no training camera sees; this is that test, of grid cells
 * against camera frusta.  The arithmetic is lab4d_amd/csrc/occvis_math.hpp, shared with the CPU twin
 * tests/host_harness/occvis/occvis_host.cpp, which the kernels equal word for word.
 *
 * Rules:
 *   VIEWS    M >= 1 views, each six world-space half-spaces: planes (M, 6, 4) fp32 = {nx, ny, nz, d}; a point x is inside a half-space iff
 *            n.x + d >= 0.  Plane order: left, right, top, bottom, near, far.
 *   CAMERA   x_cam = R x_field + t with field2cam = [R | t]; a point projects to u = fx x/z + cx, v = fy y/z + cy (Kmat = {fx, fy, cx, cy});
 *            a view of W x H pixels sees the points with -pad <= u <= W + pad, -pad <= v <= H + pad and near <= z <= far.  In the camera
 *            frame, before normalisation, (nx, ny, nz, d) =
 *              left (fx, 0, cx + pad, 0)    right (-fx, 0, W + pad - cx, 0)    top (0, fy, cy + pad, 0)    bottom (0, -fy, H + pad - cy, 0)
 *              near (0, 0, 1, -near)        far (0, 0, -1, far)
 *            (u >= -pad with z > 0 is fx x + (cx + pad) z >= 0, and so on).  Each plane is scaled to a unit normal and moved to the field
 *            frame: n_w = R^T n_c, d_w = n_c.t + d_c.  All of it in float64, rounded to fp32 once.  No far plane (far = None) is the plane
 *            (0, 0, 0, 1), which every cell passes.  (lab4d_amd.occgrid.camera_planes builds them; the kernels take the planes as given.)
 *   BOX      cell (i, j, k) of a grid with box aabb = {lo xyz, hi xyz} and G cells per axis, in the GRID indexing and bit layout of
 *            lab4d_occgrid.h: per axis, in float64, e = hi - lo, h = e / (2 G), c = lo + (2 i + 1) h (product and sum rounded on their
 *            own), then c and h rounded to fp32 once each.  (The float64 step matters: lo + (2 i + 1) h in fp32 loses |lo| ulps where the
 *            box straddles the origin and |c| is small, which no bound in terms of |c| and h covers.)
 *   SEES     view m sees a cell iff all 24 coefficients of the view are finite and, for all six planes,
 *                v = n.c + |n|.h + d >= -slack,    slack = 16 * 2^-23 * (sum_a |n_a| (|c_a| + h_a) + |d|),
 *            evaluated in fp32 as  v = ((((((nx cx + ny cy) + nz cz) + |nx| hx) + |ny| hy) + |nz| hz) + d)  and
 *            slack = 16 * 2^-23 * (((|nx| qx + |ny| qy) + |nz| qz) + |d|), q_a = |c_a| + h_a, every product and sum rounded on its own.
 *            n.c + |n|.h + d is the largest value of n.x + d over the box, so the rule keeps the box unless it lies wholly outside one
 *            half-space.  It is conservative on purpose: a box near a frustum corner may be kept although no point of it is seen, never
 *            the other way round.
 *   SLACK    with u = 2^-24 and B = sum_a |n_a| (|c_a| + h_a) + |d| (of the exact values): each of n_a, d, c_a, h_a carries one rounding
 *            (relative u; the float64 steps of BOX add 2^-52), each of the six products one, so a term n_a c_a or |n_a| h_a is off by at
 *            most 3 u of itself and d by u; each of the six additions rounds a partial sum bounded by B, u B each.  Together
 *            |v_fp32 - v_exact| <= (3 + 6) u B + O(u^2) = 4.5 * 2^-23 B.  The slack itself is B within a relative 6 u.  So a cell with
 *            v_exact >= 0 is always seen (4.5 < 16), and a cell with v_exact < -2 * slack never is.  16 keeps a factor of three in hand over
 *            the eleven roundings a looser count gives; the cost is a shell of 2^-19 B around each plane that is kept.
 *   VISIBLE  a cell's bit of vis_bits is set iff at least min_views views see it, 1 <= min_views <= M.
 *   APPLY    bits &= vis_bits; ema = 0 where the cell is invisible ("known empty", not the +inf of "nothing known yet"); n_occupied = the
 *            number of set bits of the new words.
 *
 * Both calls run on the given stream, read nothing back, allocate nothing and are capturable in a hipGraph.  Arguments are checked before any
 * launch: 1 <= M <= 2^20, 1 <= K <= 8, 2 <= G <= 256, 1 <= min_views <= M, no null pointer, planes 16-byte aligned.  (K and G need not
 * satisfy the cascade's "G even when K > 1": the levels are independent here.)
 */
#ifndef LAB4D_OCCVIS_H
#define LAB4D_OCCVIS_H

/* planes (M, 6, 4), aabbs (K, 6) -> vis_bits (K, n_words(G)) (every word rewritten, the padding bits of the last word zero), n_visible (K)
 * int32 (overwritten: the number of set bits per level).  All K levels in one launch, one lane per cell; the planes go through LDS in
 * tiles of 64 views; a wave's 64 decisions are one ballot = two words, no atomics on the words; a wave leaves the loop over the views as
 * soon as every one of its cells has min_views; n_visible is a sum of popcounts through integer atomics (order-independent). */
int lab4d_occvis_mark(const float* planes, int M, const float* aabbs, int K, int G, int min_views, uint32_t* vis_bits, int32_t* n_visible,
                      void* stream);

/* APPLY on K levels: vis_bits, bits (K, n_words(G)), ema (K, G^3), n_occupied (K) int32 (overwritten). */
int lab4d_occvis_apply(const uint32_t* vis_bits, float* ema, uint32_t* bits, int32_t* n_occupied, int K, int G, void* stream);

#endif /* LAB4D_OCCVIS_H */
