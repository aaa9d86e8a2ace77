/*
 * lab4d_meshsdf.h -- signed distance from points to a triangle mesh (included by lab4d_hip.h).
 *
 * The device counterpart of the pysdf query behind NeRF.get_init_sdf_fn (nnutils/nerf.py:217-230: `pts -> -SDF(vertices, faces)(pts)`,
 * negative inside), and the consumer of the meshes of lab4d_mesh.h.  Brute force, O(points x faces), fp32, no acceleration structure.
 * pysdf's arithmetic cannot be run where this project is built: the rules are this repository's own, parity with pysdf is unpinned.  The
 * arithmetic is lab4d_amd/csrc/meshsdf_math.hpp, shared with the CPU twin tests/host_harness/meshsdf_host.cpp; the kernels' distance, face
 * index and closest point equal the twin's bit for bit.
 *
 * Rules:
 *   VALID     a triangle (i0, i1, i2) is valid iff all three indices lie in [0, n_verts), all nine coordinates are finite, and the squared
 *             length of (b - a) x (c - a) is finite and > 0.  An invalid triangle is skipped, for the distance and for the sign.
 *   DISTANCE  the closest point of the triangle by region classification (vertex, edge or face region: Ericson, Real-Time Collision
 *             Detection, 5.1.5); every product that feeds a sum or a comparison is rounded on its own; d2 = the squared distance to that
 *             point, d = sqrt(d2) correctly rounded.  Over the faces the smallest d2 wins (a d2 that is not < +inf never wins); ties go
 *             to the lowest face index (a strict < in ascending face order, and in ascending slice order when partial results are
 *             combined).  d2, the closest point and the winning face do not depend on n_slices.
 *   SIGN      generalised winding number w = (1 / 4 pi) * sum over the valid faces of
 *             2 * atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), a, b, c = vertex - p, accumulated in fp32 in ascending
 *             face order inside a slice, slices added in ascending order.  inside iff |w| > 0.5 (either orientation of the mesh);
 *             sdf = -d inside, +d outside.  Deterministic run to run for a given n_slices; the last bits of w may differ between slice
 *             counts and from the twin (atan2f).
 *   EDGES     a point with a non-finite coordinate: sdf = NaN, face = -1, closest = the point.  No valid triangle (n_faces = 0
 *             included): sdf = +inf, face = -1, closest = the point.
 *   SLICES    slice s of n_slices covers the faces [s * n_faces / n_slices, (s + 1) * n_faces / n_slices) (integer division); a slice
 *             may be empty, any n_slices in [1, 65535] works.
 *   WORK      n_slices == 1: work is not used and may be NULL.  Otherwise n_slices * n_pts * 6 32-bit words, which must stay below 2^31
 *             (query the points in chunks beyond that): for slice s and k in 0..5 (d2, face, closest x y z, winding sum) the n_pts values
 *             at work[(s * 6 + k) * n_pts].
 *
 * Capturable in a hipGraph (no atomics, no read-back, no allocation); arguments are checked before any launch.
 */
#ifndef LAB4D_MESHSDF_H
#define LAB4D_MESHSDF_H

/* verts (n_verts, 3) fp32, faces (n_faces, 3) int32, pts (n_pts, 3) fp32 -> sdf (n_pts) fp32, face_idx (n_pts) int32 or NULL,
 * closest (n_pts, 3) fp32 or NULL.  Launch grid (ceil(n_pts / 256), n_slices), then one lane per point to fold the slices.
 * n_faces <= (2^31 - 1) / 3, n_pts < 2^31. */
int lab4d_mesh_sdf(const float* verts, const int32_t* faces, int n_verts, int n_faces, const float* pts, long n_pts, int n_slices,
                   float* work, float* sdf, int32_t* face_idx, float* closest, void* stream);

#endif /* LAB4D_MESHSDF_H */
