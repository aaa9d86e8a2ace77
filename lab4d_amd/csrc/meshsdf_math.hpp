// Signed distance from points to a triangle mesh (csrc/meshsdf.hip; contract: include/lab4d_meshsdf.h): brute force, every point against
// every face.  The device counterpart of the pysdf query behind NeRF.get_init_sdf_fn (nnutils/nerf.py:217-230); pysdf's own arithmetic
// cannot be run where this project is built, so the rules below are this repository's own and parity with pysdf is unpinned.
// Plain C++ behind LAB4D_HD (see hd_math.hpp): the kernels run these functions one lane per point, tests/host_harness/meshsdf_host.cpp
// compiles them with g++ (-ffp-contract=off) as serial loops, and the GPU suite holds the kernels' distance, face and closest point bit
// for bit to that twin.
//
// VALID     a triangle (i0, i1, i2) is valid iff all three indices lie in [0, n_verts), all nine coordinates are finite, and the squared
//           length of (b - a) x (c - a) is finite and > 0.  An invalid triangle is skipped, for the distance and for the sign.
// DISTANCE  the closest point q of the triangle by region classification (vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, face:
//           Ericson, Real-Time Collision Detection, 5.1.5, in that order: closest_reg, which the grid query of meshnear_math.hpp runs too),
//           d2 = |p - q|^2, d = sqrt(d2) correctly rounded.  Every product that feeds a sum or a comparison is rounded on its own (mul_rn, see hd_math.hpp, as for sqrt_rn); the quotients are the
//           correctly rounded division on both sides.  Over the faces the smallest d2 wins; a d2 that is not < +inf (overflow) never
//           wins.  TIES go to the lowest face index: a strict < while walking the faces in ascending order, and a strict < in ascending
//           slice order when partial results are combined.  d2, q and the winning face are therefore a pure function of the inputs,
//           whatever the partition of the faces.
// SIGN      generalised winding number (Jacobson et al. 2013; the solid angle of van Oosterom & Strackee 1983):
//             w = (1 / 4 pi) * sum over the valid faces of 2 * atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|),
//           a, b, c = vertex - p.  The code sums the atan2 terms t and multiplies once by 1 / (2 pi): doubling is exact, so that is the
//           same sum.  fp32, ascending face order inside a slice, slices added in ascending order.  inside iff |w| > 0.5 (the absolute
//           value makes the mesh's orientation irrelevant); sdf = -d inside, +d outside (nerf.py:226).  These terms are plain arithmetic
//           (the device may fuse a product into a sum) and atan2f is each side's own: the winding sum is deterministic on the device for
//           a given slice count, but not bit-equal to the twin, nor between slice counts.
// EDGES     a point with a non-finite coordinate: sdf = NaN, face = -1, closest = the point.  No valid triangle (n_faces = 0 included):
//           sdf = +inf, face = -1, closest = the point.
// SLICES    slice s of n covers the faces [s * F / n, (s + 1) * F / n) (integer division in 64 bits); it may be empty.
#pragma once
#include "hd_math.hpp"

namespace lab4d_msdf {
using lab4d_rn::div_rn;
using lab4d_rn::finite_f;
using lab4d_rn::inf_f;
using lab4d_rn::mul_rn;
using lab4d_rn::nan_f;
using lab4d_rn::sqrt_rn;

constexpr int kWorkWords = 6;  // per (slice, point): d2, face, closest xyz, winding sum

LAB4D_HD long slice_lo(int s, int n_faces, int n_slices) { return (long)s * n_faces / n_slices; }

LAB4D_HD float dot_rn(float ax, float ay, float az, float bx, float by, float bz) { return mul_rn(ax, bx) + mul_rn(ay, by) + mul_rn(az, bz); }

// n = u x w, every product rounded on its own.  With u = b - a, w = c - a: the face normal of VALID, of the mesh ray caster's front side and of
// the nearest-point query's pseudonormals.
LAB4D_HD void cross_rn(float ux, float uy, float uz, float wx, float wy, float wz, float& nx, float& ny, float& nz) {
  nx = mul_rn(uy, wz) - mul_rn(uz, wy), ny = mul_rn(uz, wx) - mul_rn(ux, wz), nz = mul_rn(ux, wy) - mul_rn(uy, wx);
}

// v = the nine coordinates a, b, c of a triangle whose indices were in range
LAB4D_HD bool tri_valid(const float* v) {
  for (int k = 0; k < 9; ++k)
    if (!finite_f(v[k])) return false;
  float nx, ny, nz;
  cross_rn(v[3] - v[0], v[4] - v[1], v[5] - v[2], v[6] - v[0], v[7] - v[1], v[8] - v[2], nx, ny, nz);
  const float n2 = dot_rn(nx, ny, nz, nx, ny, nz);
  return finite_f(n2) && n2 > 0.f;
}

// Gather face f: the nine coordinates into v; returns VALID
LAB4D_HD bool load_tri(const float* verts, const int32_t* faces, int n_verts, long f, float* v) {
  const int32_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_verts || i1 >= n_verts || i2 >= n_verts) {
    for (int k = 0; k < 9; ++k) v[k] = 0.f;
    return false;
  }
  for (int k = 0; k < 3; ++k) {
    v[k] = verts[3 * (long)i0 + k];
    v[3 + k] = verts[3 * (long)i1 + k];
    v[6 + k] = verts[3 * (long)i2 + k];
  }
  return tri_valid(v);
}

// which feature of the triangle holds the closest point (the nearest-point query of meshnear_math.hpp reports it and signs by it)
enum Region { kFace = 0, kEdgeAB = 1, kEdgeAC = 2, kEdgeBC = 3, kVertA = 4, kVertB = 5, kVertC = 6 };

// closest point of triangle (a, b, c) to p -> (qx, qy, qz) and the region it lies in; returns d2.  Scalars, not arrays: everything stays in
// registers on the device.  The ONE statement of DISTANCE: the brute-force query and the grid query both run it.
LAB4D_HD float closest_reg(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                           float& qx, float& qy, float& qz, int32_t& region) {
  const float abx = bx - ax, aby = by - ay, abz = bz - az;
  const float acx = cx - ax, acy = cy - ay, acz = cz - az;
  const float apx = px - ax, apy = py - ay, apz = pz - az;
  const float d1 = dot_rn(abx, aby, abz, apx, apy, apz), d2 = dot_rn(acx, acy, acz, apx, apy, apz);
  const float bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const float d3 = dot_rn(abx, aby, abz, bpx, bpy, bpz), d4 = dot_rn(acx, acy, acz, bpx, bpy, bpz);
  const float cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const float d5 = dot_rn(abx, aby, abz, cpx, cpy, cpz), d6 = dot_rn(acx, acy, acz, cpx, cpy, cpz);
  const float vc = mul_rn(d1, d4) - mul_rn(d3, d2);
  const float vb = mul_rn(d5, d2) - mul_rn(d1, d6);
  const float va = mul_rn(d3, d6) - mul_rn(d5, d4);
  if (d1 <= 0.f && d2 <= 0.f) {
    qx = ax, qy = ay, qz = az, region = kVertA;
  } else if (d3 >= 0.f && d4 <= d3) {
    qx = bx, qy = by, qz = bz, region = kVertB;
  } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
    const float t = div_rn(d1, d1 - d3);
    qx = ax + mul_rn(t, abx), qy = ay + mul_rn(t, aby), qz = az + mul_rn(t, abz), region = kEdgeAB;
  } else if (d6 >= 0.f && d5 <= d6) {
    qx = cx, qy = cy, qz = cz, region = kVertC;
  } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
    const float t = div_rn(d2, d2 - d6);
    qx = ax + mul_rn(t, acx), qy = ay + mul_rn(t, acy), qz = az + mul_rn(t, acz), region = kEdgeAC;
  } else if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {
    const float t = div_rn(d4 - d3, (d4 - d3) + (d5 - d6));
    qx = bx + mul_rn(t, cx - bx), qy = by + mul_rn(t, cy - by), qz = bz + mul_rn(t, cz - bz), region = kEdgeBC;
  } else {
    const float sum = va + vb + vc;
    const float v = div_rn(vb, sum), w = div_rn(vc, sum);
    qx = ax + mul_rn(abx, v) + mul_rn(acx, w), qy = ay + mul_rn(aby, v) + mul_rn(acy, w), qz = az + mul_rn(abz, v) + mul_rn(acz, w), region = kFace;
  }
  const float ex = px - qx, ey = py - qy, ez = pz - qz;
  return dot_rn(ex, ey, ez, ex, ey, ez);
}

// closest_reg without the region
LAB4D_HD float closest_d2(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                          float& qx, float& qy, float& qz) {
  int32_t region;
  return closest_reg(px, py, pz, ax, ay, az, bx, by, bz, cx, cy, cz, qx, qy, qz, region);
}

// half the signed solid angle of the triangle seen from p: atan2(det, ...) of SIGN
LAB4D_HD float winding_term(float px, float py, float pz, float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
  ax -= px, ay -= py, az -= pz;
  bx -= px, by -= py, bz -= pz;
  cx -= px, cy -= py, cz -= pz;
  const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz), lc = sqrtf(cx * cx + cy * cy + cz * cz);
  const float det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
  const float den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb;
  return atan2f(det, den);
}

// the running result of one point over a range of faces
struct Best {
  float d2, qx, qy, qz, wsum;
  int32_t face;
};

LAB4D_HD Best best_init(float px, float py, float pz) { return Best{inf_f(), px, py, pz, 0.f, -1}; }

// one valid face, visited in ascending order
LAB4D_HD void best_visit(Best& r, float px, float py, float pz, const float* v, int32_t face) {
  float qx, qy, qz;
  const float d2 = closest_d2(px, py, pz, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], qx, qy, qz);
  if (d2 < r.d2) r.d2 = d2, r.qx = qx, r.qy = qy, r.qz = qz, r.face = face;
  r.wsum += winding_term(px, py, pz, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]);
}

// a later slice's result folded into an earlier one's
LAB4D_HD void best_merge(Best& r, const Best& s) {
  if (s.d2 < r.d2) r.d2 = s.d2, r.qx = s.qx, r.qy = s.qy, r.qz = s.qz, r.face = s.face;
  r.wsum += s.wsum;
}

LAB4D_HD bool point_finite(float px, float py, float pz) { return finite_f(px) && finite_f(py) && finite_f(pz); }

// the final outputs of a point from its folded result
LAB4D_HD float best_sdf(const Best& r, bool pt_ok) {
  if (!pt_ok) return nan_f();
  if (r.face < 0) return inf_f();
  const float d = sqrt_rn(r.d2);
  const float w = r.wsum * 0.15915494309189535f;  // 1 / (2 pi)
  return fabsf(w) > 0.5f ? -d : d;
}

}  // namespace lab4d_msdf
