/*
 * lab4d_meshray.h -- ray casting against a triangle mesh through a uniform face grid (included by lab4d_hip.h).
 *
 * The proxy geometry is a welded triangle mesh on the device (lab4d_mesh.h); lab4d_meshsdf.h answers a point's distance to it by brute force.
 * This answers the renderer's question -- where does a ray hit it first -- and builds the first acceleration structure over faces: a per-ray
 * sampling range from the proxy (first and last hit), a depth / mask / face-id map for a camera.  Not in the reference (no ray caster): the
 * rules are this repository's own, parity is unpinned, the truth of the tests is numpy float64.  The arithmetic is
 * lab4d_amd/csrc/meshray_math.hpp over hd_math.hpp (products, sums and quotients rounded on their own, no contraction) and meshsdf_math.hpp
 * (VALID), shared with the CPU twin tests/host_harness/meshray/meshray_host.cpp.  fp32 throughout, double only where INTERSECT says so.
 *
 * Rules (ray o + t * d, t in [t0, t1] in units of d, d of any length; aabb = {lo, hi}):
 *   VALID      a face is valid iff its three indices lie in [0, n_verts), its nine coordinates are finite and |(b - a) x (c - a)|^2 is finite
 *              and > 0 (lab4d_meshsdf.h).  An invalid face is never hit and never binned.
 *   RAY        len = |d| as lab4d_packed.h rounds it.  REJECT: a non-finite o, d, t0 or t1, t0 > t1, len == 0 or a box without extent:
 *              face = -1, t = t0, u = v = 0, front = 0, n_tests = 0.  A ray that hits nothing gets the same values, with its own n_tests.
 *   CLIP       [t0, t1] is cut to the box with the slab test of lab4d_hashtrace.h (CLIP): a parallel axis is always or never satisfied, no
 *              inf or NaN arithmetic.  An empty clip: a miss without a test.  The mesh is cut to the box: a face test accepts t in the clipped
 *              range [t_enter, t_exit] (the whole of it, not the span of the cell the test is made in).  With a box that holds the mesh with
 *              a margin -- the Python layer's default -- that is t0 <= t <= t1.
 *   INTERSECT  the watertight test of Woop, Benthin and Wald 2013: kz = argmax |d_k| (ties to the lowest axis), kx = (kz + 1) % 3,
 *              ky = (kx + 1) % 3, swapped if d[kz] < 0; Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz]; per vertex P' = P - o,
 *              Px = P'[kx] - Sx P'[kz], Py = P'[ky] - Sy P'[kz]; U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax, every product
 *              rounded on its own; if one of them is exactly 0 all three are formed in double from the same float operands (and rounded to
 *              float).  One negative and one positive: a miss.  det = (U + V) + W, det == 0: a miss.
 *              T = (U (Sz A'[kz]) + V (Sz B'[kz])) + W (Sz C'[kz]), t = T / det, a hit iff t lies in the range.  No back-face culling:
 *              front = 1 iff the ray meets the side (b - a) x (c - a) points to (det > 0).  u = V / det is b's barycentric weight,
 *              v = W / det is c's.
 *   FIRST HIT  the smallest t over the valid faces wins, ties go to the lowest face index.  The result does not depend on the grid, on G or
 *              on the order of any list; G = 1 is the brute-force statement of the rule.
 *   GRID       G^3 cells, 1 <= G <= 128; cell (ix, iy, iz) has index ix + G (iy + G iz); grid coordinate g = ((x - lo) / (hi - lo)) * G.  A
 *              valid face is listed in the cells [floor(g_min - 2^-10), floor(g_max + 2^-10)] of its own bounding box per axis, clamped to the
 *              grid; a face wholly outside the box is listed nowhere and cannot be hit.  The pad is 75 x the fp32 error of o + t d at box
 *              scale (1.3e-5 of a cell at G = 128): rounding in the traversal cannot lose a hit.
 *   TRAVERSAL  Amanatides-Woo with integer cell steps from the cell of o + t_enter d; the parameter of a cell wall is recomputed from the
 *              integer index at every step.  In a cell every listed face is tested, the best (t, face) under the tie rule is kept; the walk
 *              stops when the ray leaves the cell behind the best t (or behind t_exit), or leaves the grid.  n_tests = the face tests the ray
 *              made: a measurement, not part of the parity between grid sizes.
 *
 * Buffers (the caller's; sizes in 32-bit words, n_cells = G^3):
 *   tris        12 * n_faces floats   the packed faces: {a xyz, valid}, {b xyz, 0}, {c xyz, 0}, 16-byte aligned
 *   cell_start  n_cells + 1 ints      the exclusive prefix sum of the cells' list lengths; cell_start[n_cells] = the length of cell_list
 *   work        n_cells + ceil(n_cells / 1024) ints   the per-cell counts (count) / cursors (fill) and the scan's block sums
 *   total       1 int                 the length of cell_list, left on the device by the count; the host reads it once and allocates
 *   cell_list   *total ints           face indices, cell after cell; the order within a cell is unspecified
 *
 * lab4d_meshgrid_count packs the faces, counts with integer atomics (the totals are deterministic) and scans; lab4d_meshgrid_fill claims the
 * slots with integer atomics.  lab4d_mesh_raycast: one lane per ray, 256 per workgroup, grid-stride over at most 2,048 workgroups, no
 * atomics, no read-back, no allocation: capturable in a hipGraph.  Arguments are checked before any launch: 1 <= G <= 128,
 * 0 <= n_faces <= 2^31 / 12, n_verts >= 0, 0 <= R < 2^31, n_list >= 0, every pointer that is read or written non-NULL.  n_faces == 0 makes
 * count and fill successful no-ops and every ray of the cast a miss (the grid buffers are not looked at and may be NULL); R == 0 is a
 * successful no-op (the per-ray arrays may be NULL).
 */
#ifndef LAB4D_MESHRAY_H
#define LAB4D_MESHRAY_H

/* verts (n_verts,3), faces (n_faces,3) int32, aabb (6) -> tris, cell_start, *total; work is scratch. */
int lab4d_meshgrid_count(const float* verts, const int32_t* faces, int n_verts, int n_faces, const float* aabb, int G, float* tris,
                         int32_t* cell_start, int32_t* work, int32_t* total, void* stream);
/* tris, cell_start as the count left them, n_list = *total as the host read it -> cell_list (n_list); work is scratch. */
int lab4d_meshgrid_fill(const float* tris, int n_faces, const float* aabb, int G, const int32_t* cell_start, int32_t* work, int n_list,
                        int32_t* cell_list, void* stream);
/* The packing of the count alone: verts, faces -> tris; the lists stay as they are.  For vertices that move while every face keeps touching
 * the cells that list it (always so at G = 1 for faces that stay in the box).  No atomics, no read-back: capturable. */
int lab4d_meshgrid_pack(const float* verts, const int32_t* faces, int n_verts, int n_faces, float* tris, void* stream);
/* origin, dir (R,3), t_range (R,2) = {t0, t1} -> t, u, v (R) float, face, front, n_tests (R) int32. */
int lab4d_mesh_raycast(const float* origin, const float* dir, const float* t_range, long R, const float* tris, int n_faces, const float* aabb, int G,
                       const int32_t* cell_start, const int32_t* cell_list, float* t, int32_t* face, float* u, float* v, int32_t* front,
                       int32_t* n_tests, void* stream);

#endif /* LAB4D_MESHRAY_H */
