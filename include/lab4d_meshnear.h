/*
 * lab4d_meshnear.h -- closest point and signed distance from points to a triangle mesh through the face grid (included by lab4d_hip.h).
 *
 * lab4d_meshsdf.h answers a point's distance to the proxy mesh by brute force, every point against every face, and takes its sign from a sum
 * over all faces.  This answers the same question through the face grid of lab4d_meshray.h: a point tests the faces listed near it, and the sign
 * is a local question once the closest feature is known.  The arithmetic is lab4d_amd/csrc/meshnear_math.hpp over hd_math.hpp, meshsdf_math.hpp
 * and meshray_math.hpp (all three unchanged), shared with the CPU twin tests/host_harness/meshnear/meshnear_host.cpp.  fp32 throughout.
 *
 * Rules (p a query point, aabb = {lo, hi}, the grid buffers as lab4d_meshgrid_count / _fill left them):
 *   DISTANCE   lab4d_meshsdf.h's: the closest point q of a face by region classification in Ericson's order, every product rounded on its own,
 *              d2 = |p - q|^2, d = sqrt(d2) correctly rounded.  TIES: the smallest d2 wins, ties go to the lowest face index; a d2 that is not
 *              < +inf never wins.  VALID: lab4d_meshsdf.h's; an invalid face is listed nowhere, never wins and is never incident.  EDGES: a
 *              point with a non-finite coordinate: sdf = d2 = NaN, face = region = -1, closest = the point, n_tests = 0.  No valid face listed
 *              (n_faces = 0 included): sdf = d2 = +inf, face = region = -1, closest = the point.
 *              d2, q and the face are word for word those of lab4d_mesh_sdf at every G, provided the box holds the mesh (a face wholly outside
 *              the box is listed nowhere: the Python layer refuses such a grid).  G = 1 is the brute-force statement of the rule.
 *   REGION     which feature of the winning face q lies on: 0 the face, 1 / 2 / 3 the edge ab / ac / bc, 4 / 5 / 6 the vertex a / b / c.
 *   SEARCH     c0 = the cell of p: floor of 7j's grid coordinate ((p - lo) / (hi - lo)) * G per axis, clamped into [0, G - 1] (a point outside
 *              the box starts at the nearest cell).  Shell r = the cells at Chebyshev index distance exactly r from c0 that lie inside the grid;
 *              shells r = 0, 1, 2, ... are visited, each cell once, and in a visited cell every listed face is tested (a face listed in several
 *              cells is tested again: the minimum under the tie rule is idempotent).  After shell r a side of the index cube [c0 - r, c0 + r] is
 *              OPEN if grid cells lie beyond it; bound_r = the smallest, over the open sides, of the distance from p to the side's plane minus
 *              the axis' margin, clamped at 0.  The plane is lo + (k / G) * (hi - lo) from the integer index k, as 7j's walls are.  The walk
 *              stops when no side is open, or when best d2 < bound_r^2, strictly.
 *   MARGIN     per axis: 2^-6 (hi - lo) / G + 2^-16 (|p - lo| + |p - hi|) + 2^-20 (|lo| + |hi|).
 *              Why a stop is exact.  A face that no visited cell lists has, on some axis, an index range disjoint from [c0 - r, c0 + r], so it
 *              lies beyond an open side: floor(g_max + 2^-10) < k or floor(g_min - 2^-10) >= k puts its grid coordinates at least 7j's listing
 *              pad beyond k, so the pad works for the stop rule and is not charged to the margin.  What the margin pays for:
 *              (1) the plane: lo + (k / G) ext carries two roundings at the scale of the box' coordinates, <= 2^-23 (|lo| + |hi|), and the grid
 *              coordinate of a vertex three (difference, quotient, product), <= 3 * 2^-24 * G cells = 2.3e-5 of a cell at G = 128: the third and
 *              the first term (2^-6 of a cell is 68 x the pad's own 75 x cover of 7j).
 *              (2) closest_d2 at the point's scale.  With D = |p - x| for a point x of the face, the computed d2 is the square of the distance
 *              to a computed q whose coordinates carry a few roundings at the scale of the face and of p: |d2 - D^2| <= c eps D (|p| + |x|)
 *              with c a few tens (lab4d_meshsdf.h bounds it by 64 eps L^2), and a tangential error of q enters in second order only.  The
 *              second term grows with the point's distance from the box in the same way: the stop compares d2 against (D_plane - m)^2 with
 *              m >= 2^-16 (|p - lo| + |p - hi|) >= 2^-16 D_plane, a relative slack of 2^-15 in d2 = 512 eps, eight times the bound above.
 *              A margin that swallows the bound only makes the walk go on: that is still exact.  A point far outside the box sees small
 *              distances to the planes of the axes on which it lies beside the box and visits every cell.
 *   SIGN       not the winding number: the pseudonormal of the closest feature (Baerentzen and Aanaes 2005), s = (p - q) . n.
 *              Face region: n = (b - a) x (c - a) of the winning face.  Edge region: n = the sum of the unit normals of the incident faces.
 *              Vertex region: n = the sum of angle * unit normal of the incident faces, angle = atan2f(|e1 x e2|, e1 . e2) between the face's
 *              two edges at that vertex.  INCIDENT: a listed valid face of q's cell (the same grid coordinate, clamped) one of whose vertices
 *              equals the feature's vertex in all three coordinates (an edge: both of its ends).  Coordinates, not indices: the packed faces
 *              are enough and an unwelded mesh works.  Every incident face contains the feature, hence q, so q's cell lists it whenever the
 *              box holds the mesh.  The sum runs in ascending face index whatever the order of the list.  Unit normals and the edge sum use
 *              the correctly rounded root and quotient and individually rounded products: face and edge regions are bit-equal between the
 *              device and the twin; a vertex region's atan2f is each side's own (as lab4d_meshsdf.h's winding term is).
 *              orient = +1 / -1 says whether (b - a) x (c - a) points outward / inward.  sdf = -d iff orient * s < 0; s == 0 is outside.
 *              On an open mesh this is "the side of the nearest feature"; it differs from lab4d_meshsdf.h's |w| > 0.5 there by design.  On
 *              closed, consistently oriented meshes the two agree away from the surface.  sign_mode = 0 skips the sign: sdf = +d.
 *   N_TESTS    the face tests of the distance walk (not the sign's loads): a measurement; it depends on G, not on the order of the lists.
 *
 * lab4d_mesh_closest: one lane per point, 256 per workgroup, grid-stride over at most 2,048 workgroups; no atomics, no read-back, no
 * allocation: capturable in a hipGraph.  Arguments are checked before any launch: 1 <= G <= 128, 0 <= n_faces <= 2^31 / 12, 0 <= N < 2^31,
 * sign_mode in {0, 1}, orient in {-1, +1}, aabb non-NULL, tris and cell_start non-NULL when n_faces > 0 (cell_list is NULL when the lists are empty), pts and sdf
 * non-NULL when N > 0.  Each of d2, face, closest, region and n_tests may be NULL.  n_faces == 0: the grid buffers are not looked at and may be NULL.
 * N == 0 is a successful no-op.
 */
#ifndef LAB4D_MESHNEAR_H
#define LAB4D_MESHNEAR_H

/* pts (N,3) -> sdf, d2 (N) float, face, region, n_tests (N) int32, closest (N,3) float. */
int lab4d_mesh_closest(const float* pts, long N, const float* tris, int n_faces, const float* aabb, int G, const int32_t* cell_start,
                       const int32_t* cell_list, int sign_mode, int orient, float* sdf, float* d2, int32_t* face, float* closest,
                       int32_t* region, int32_t* n_tests, void* stream);

#endif /* LAB4D_MESHNEAR_H */
