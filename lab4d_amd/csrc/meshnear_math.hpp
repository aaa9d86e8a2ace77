// Closest point and signed distance from points to a triangle mesh through the face grid of meshray_math.hpp (csrc/meshnear.hip; contract:
// include/lab4d_meshnear.h, where every rule is written down once).  Plain C++ behind LAB4D_HD on hd_math.hpp's individually rounded products,
// sums, quotients and roots, on meshsdf_math.hpp (closest_reg and its Region, cross_rn, dot_rn, point_finite) and on meshray_math.hpp (Quad,
// load_face, cell_of, plane_at, the packed faces and the lists).  The kernel runs find_nearest one lane per point, the CPU twin
// tests/host_harness/meshnear/meshnear_host.cpp compiles the same text with g++ (-ffp-contract=off) as a serial loop, and the GPU suite holds the kernel's d2, face, closest point and region bit for bit
// to that twin, and the sign wherever the region is a face or an edge (a vertex region's atan2f is each side's own, as the winding term of
// meshsdf_math.hpp is).
//
// DISTANCE, TIES, VALID, EDGES  meshsdf_math.hpp's.  closest_reg is the brute-force query's own function (closest_d2 is it without the region);
//            the smallest d2 wins, ties go to the lowest face index whatever the order of the walk (d2 < best, or d2 == best and f < best's
//            face; a d2 that is not < +inf never wins).
// REGION     0 face, 1 / 2 / 3 edge ab / ac / bc, 4 / 5 / 6 vertex a / b / c of the winning face; -1 without one.
// SEARCH     shells of cells around the cell of p, see find_nearest and the header's error argument for the margin.
// SIGN       the pseudonormal of the closest feature (Baerentzen & Aanaes 2005), from the listed faces of q's cell: see feature_side.
#pragma once
#include "meshray_math.hpp"

namespace lab4d_mnear {
namespace msdf = lab4d_msdf;
namespace mr = lab4d_mray;
using lab4d_rn::add_rn;
using lab4d_rn::div_rn;
using lab4d_rn::inf_f;
using lab4d_rn::mul_rn;
using lab4d_rn::nan_f;
using lab4d_rn::sqrt_rn;
using mr::cell_of;
using mr::load_face;
using mr::plane_at;
using msdf::closest_reg;
using msdf::cross_rn;
using msdf::dot_rn;

constexpr int kBlock = 256;                        // points per workgroup
constexpr float kMarginCell = 0.015625f;           // 2^-6 of a cell's width
constexpr float kMarginReach = 1.52587890625e-5f;  // 2^-16 of |p - lo| + |p - hi|
constexpr float kMarginBox = 9.5367431640625e-7f;  // 2^-20 of |lo| + |hi|

struct Found {
  float sdf, d2, qx, qy, qz;
  int32_t face, region, n_tests, n_cells;  // n_cells: the cells the walk visited (a measurement, kept by the twin alone)
};

// bound_r of one axis: the distance from p to the nearer OPEN side of [c0 - r, c0 + r] (a side with grid cells beyond it) minus the margin;
// *open is set when the axis has an open side.  The result may be negative or NaN (an overflowing margin): the caller clamps, and stops on
// neither.
LAB4D_HD float axis_bound(float p, float lo, float hi, int G, int c0, int r, float b, bool* open) {
  const float ext = hi - lo;
  const float margin = add_rn(add_rn(mul_rn(kMarginCell, div_rn(ext, (float)G)), mul_rn(kMarginReach, fabsf(p - lo) + fabsf(p - hi))),
                              mul_rn(kMarginBox, fabsf(lo) + fabsf(hi)));
  if (c0 - r > 0) {
    const float d = (p - plane_at(c0 - r, lo, ext, G)) - margin;
    b = d < b ? d : (d == d ? b : d), *open = true;  // (the minimum; a NaN stays)
  }
  if (c0 + r < G - 1) {
    const float d = (plane_at(c0 + r + 1, lo, ext, G) - p) - margin;
    b = d < b ? d : (d == d ? b : d), *open = true;
  }
  return b;
}

// the three unit-length components of (b - a) x (c - a): rounded products, the correctly rounded root and quotients
LAB4D_HD void unit_normal(const mr::Quad& a, const mr::Quad& b, const mr::Quad& c, float& nx, float& ny, float& nz) {
  float cx, cy, cz;
  cross_rn(b.x - a.x, b.y - a.y, b.z - a.z, c.x - a.x, c.y - a.y, c.z - a.z, cx, cy, cz);
  const float len = sqrt_rn(dot_rn(cx, cy, cz, cx, cy, cz));
  nx = div_rn(cx, len), ny = div_rn(cy, len), nz = div_rn(cz, len);
}

LAB4D_HD bool same_point(const mr::Quad& v, float x, float y, float z) { return v.x == x && v.y == y && v.z == z; }

// the interior angle at `at` between the directions to u and w: atan2f(|e1 x e2|, e1 . e2), each side's own atan2f
LAB4D_HD float corner_angle(const mr::Quad& at, const mr::Quad& u, const mr::Quad& w) {
  const float e1x = u.x - at.x, e1y = u.y - at.y, e1z = u.z - at.z;
  const float e2x = w.x - at.x, e2y = w.y - at.y, e2z = w.z - at.z;
  float cx, cy, cz;
  cross_rn(e1x, e1y, e1z, e2x, e2y, e2z, cx, cy, cz);
  return atan2f(sqrt_rn(dot_rn(cx, cy, cz, cx, cy, cz)), dot_rn(e1x, e1y, e1z, e2x, e2y, e2z));
}

// SIGN: s = (p - q) . n for the closest feature of the winning face.  Face region: n = (b - a) x (c - a), not normalised.  Edge and vertex
// regions: the sum over the INCIDENT faces -- the listed valid faces of q's cell that have a vertex equal in all three coordinates to the
// feature's vertex (for an edge: to both of its ends) -- of their unit normals (an edge) or of angle x unit normal (a vertex), accumulated in
// ascending face index by repeated selection of the smallest incident index above the last one: the sum does not depend on the order of the
// cell's list.  A pass costs a face load per entry that can still be the next one.
LAB4D_HD float feature_side(float px, float py, float pz, const Found& r, const float* aabb, int G, const mr::Quad* rec, const int32_t* cell_start,
                            const int32_t* cell_list) {
  mr::Quad wa, wb, wc;
  load_face(rec, r.face, wa, wb, wc);
  const float ex = px - r.qx, ey = py - r.qy, ez = pz - r.qz;
  if (r.region == msdf::kFace) {
    float nx, ny, nz;
    cross_rn(wb.x - wa.x, wb.y - wa.y, wb.z - wa.z, wc.x - wa.x, wc.y - wa.y, wc.z - wa.z, nx, ny, nz);
    return dot_rn(ex, ey, ez, nx, ny, nz);
  }
  // the feature's one or two vertices, by selects
  const bool edge = r.region <= msdf::kEdgeBC;
  const bool first_a = r.region == msdf::kEdgeAB || r.region == msdf::kEdgeAC || r.region == msdf::kVertA;
  const bool first_b = r.region == msdf::kEdgeBC || r.region == msdf::kVertB;
  const mr::Quad v0 = first_a ? wa : (first_b ? wb : wc);
  const mr::Quad v1 = r.region == msdf::kEdgeAB ? wb : wc;  // (an edge's other end; unused for a vertex)
  const int cx = cell_of(r.qx, aabb[0], aabb[3] - aabb[0], G), cy = cell_of(r.qy, aabb[1], aabb[4] - aabb[1], G),
            cz = cell_of(r.qz, aabb[2], aabb[5] - aabb[2], G);
  const int cell = cx + G * (cy + G * cz);  // (G <= 128: below 2^21; 3 f + 2 < 2^29 for n_faces <= 2^31 / 12)
  const int32_t lo = cell_start[cell], hi = cell_start[cell + 1];
  float nx = 0.f, ny = 0.f, nz = 0.f;
  int32_t last = -1;
  for (;;) {
    int32_t next = 2147483647;
    for (int32_t j = lo; j < hi; ++j) {
      const int32_t f = cell_list[j];
      if (!(f > last && f < next)) continue;
      mr::Quad a, b, c;
      load_face(rec, f, a, b, c);
      const bool has0 = same_point(a, v0.x, v0.y, v0.z) || same_point(b, v0.x, v0.y, v0.z) || same_point(c, v0.x, v0.y, v0.z);
      const bool has1 = !edge || same_point(a, v1.x, v1.y, v1.z) || same_point(b, v1.x, v1.y, v1.z) || same_point(c, v1.x, v1.y, v1.z);
      if (a.w != 0.f && has0 && has1) next = f;
    }
    if (next == 2147483647) break;
    last = next;
    mr::Quad a, b, c;
    load_face(rec, next, a, b, c);
    float ux, uy, uz;
    unit_normal(a, b, c, ux, uy, uz);
    if (edge) {
      nx = add_rn(nx, ux), ny = add_rn(ny, uy), nz = add_rn(nz, uz);
    } else {  // the face's corner at the vertex: the first of a, b, c that equals it
      const bool at_a = same_point(a, v0.x, v0.y, v0.z), at_b = same_point(b, v0.x, v0.y, v0.z);
      const mr::Quad at = at_a ? a : (at_b ? b : c), u = at_a ? b : (at_b ? c : a), w = at_a ? c : (at_b ? a : b);
      const float ang = corner_angle(at, u, w);
      nx = add_rn(nx, mul_rn(ang, ux)), ny = add_rn(ny, mul_rn(ang, uy)), nz = add_rn(nz, mul_rn(ang, uz));
    }
  }
  return dot_rn(ex, ey, ez, nx, ny, nz);
}

// One point against the grid.  tris: n_faces packed faces; cell_start (G^3 + 1), cell_list: the lists (not looked at when n_faces == 0).
// sign_mode 0: sdf = +d; 1: sdf = -d iff orient * s < 0.  Every member of the result is set.
LAB4D_HD Found find_nearest(float px, float py, float pz, const float* aabb, int G, const float* tris, int n_faces, const int32_t* cell_start,
                            const int32_t* cell_list, int sign_mode, int orient) {
  Found r;
  r.sdf = inf_f(), r.d2 = inf_f(), r.qx = px, r.qy = py, r.qz = pz, r.face = -1, r.region = -1, r.n_tests = 0, r.n_cells = 0;
  if (!msdf::point_finite(px, py, pz)) {
    r.sdf = nan_f(), r.d2 = nan_f();
    return r;
  }
  if (n_faces == 0) return r;
  const mr::Quad* rec = (const mr::Quad*)tris;
  const int c0x = cell_of(px, aabb[0], aabb[3] - aabb[0], G), c0y = cell_of(py, aabb[1], aabb[4] - aabb[1], G),
            c0z = cell_of(pz, aabb[2], aabb[5] - aabb[2], G);
  // One flat loop over the cells of shell after shell (not a nest per axis: a lane that has cells left never waits for a row or a slab of
  // another lane's cube to end).  An iteration either visits the cell (x, y, z) and moves along the row -- a whole row where y or z lies on the
  // shell, else the row's two ends --, or moves to the next row, the next slab, and after the last slab of shell s tries the stop rule.
  int s = 0, x = c0x, y = c0y, z = c0z;
  for (;;) {
    const int xe = c0x + s, x1 = xe < G - 1 ? xe : G - 1;
    const bool full = z - c0z == s || c0z - z == s || y - c0y == s || c0y - y == s;
    if (x <= x1) {
      const int cell = x + G * (y + G * z);
      const int32_t lo = cell_start[cell], hi = cell_start[cell + 1];
      ++r.n_cells;
      for (int32_t j = lo; j < hi; ++j) {
        const int32_t f = cell_list[j];
        mr::Quad a, b, c;
        load_face(rec, f, a, b, c);
        float qx, qy, qz;
        int32_t region;
        const float d2 = closest_reg(px, py, pz, a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, qx, qy, qz, region);
        ++r.n_tests;
        if (a.w != 0.f && (d2 < r.d2 || (d2 == r.d2 && f < r.face))) r.d2 = d2, r.qx = qx, r.qy = qy, r.qz = qz, r.face = f, r.region = region;
      }
      x = full ? x + 1 : (x < xe ? xe : xe + 1);
      continue;
    }
    ++y;
    if (y > (c0y + s < G - 1 ? c0y + s : G - 1)) ++z, y = c0y - s > 0 ? c0y - s : 0;
    if (z > (c0z + s < G - 1 ? c0z + s : G - 1)) {  // shell s is done
      bool open = false;
      float bound = axis_bound(px, aabb[0], aabb[3], G, c0x, s, inf_f(), &open);
      bound = axis_bound(py, aabb[1], aabb[4], G, c0y, s, bound, &open);
      bound = axis_bound(pz, aabb[2], aabb[5], G, c0z, s, bound, &open);
      if (!open) break;                                       // no side is open: every cell has been visited
      if (bound > 0.f && r.d2 < mul_rn(bound, bound)) break;  // (bound_r clamped at 0; a NaN bound never stops the walk)
      ++s;
      z = c0z - s > 0 ? c0z - s : 0, y = c0y - s > 0 ? c0y - s : 0;
    }
    const bool row = z - c0z == s || c0z - z == s || y - c0y == s || c0y - y == s;
    x = row ? (c0x - s > 0 ? c0x - s : 0) : (c0x - s >= 0 ? c0x - s : c0x + s);  // (both ends outside the grid: an empty row, left at once)
  }
  if (r.face < 0) return r;  // no listed valid face: +inf
  const float d = sqrt_rn(r.d2);
  r.sdf = d;
  if (sign_mode != 0) {
    const float s = feature_side(px, py, pz, r, aabb, G, rec, cell_start, cell_list);
    if ((orient < 0 ? -s : s) < 0.f) r.sdf = -d;
  }
  return r;
}

}  // namespace lab4d_mnear
