// Ray casting against a triangle mesh through a uniform face grid (csrc/meshray.hip; contract: include/lab4d_meshray.h).  Plain C++ behind
// LAB4D_HD on hd_math.hpp's individually rounded products, sums and quotients (no contraction anywhere that decides a result) and on
// meshsdf_math.hpp's VALID rule (tri_valid / load_tri) and on ray_math.hpp's RAY, REJECT and CLIP (dir_length, point_at, clip_ray: shared with
// the sphere tracer).  The grid's own helpers (grid_coord, cell_of, plane_at, load_face) are stated here once for the ray caster and for the
// nearest-point query of meshnear_math.hpp.  The kernels run these functions one lane per face or per ray, the CPU twin
// tests/host_harness/meshray/meshray_host.cpp compiles them with g++ (-ffp-contract=off) as serial loops, and the GPU suite holds the kernel's
// t, face, u, v and front bit for bit to that twin.  The reference has no ray caster: the rules are this repository's own.
//
// VALID      meshsdf_math.hpp: indices in [0, n_verts), nine finite coordinates, |(b - a) x (c - a)|^2 finite and > 0.  An invalid face is
//            never hit and never binned.  A face is PACKED once as three 16-byte words {a xyz, valid}, {b xyz, 0}, {c xyz, 0}.
// RAY        ray_math.hpp's: o + t * d, t in [t0, t1] in units of d, d of any length; len = |d| (dir_length).  REJECT (clip_ray's code 0): a
//            non-finite o, d, t0 or t1, t0 > t1, len == 0, or a box without extent: face = -1, t = t0, u = v = 0, front = 0, n_tests = 0.
// CLIP       ray_math.hpp's clip_ray cuts [t0, t1] to the box, every reject before the first slab.  An empty clip (code 1) is a MISS without a
//            test.  Otherwise (code 2) t_enter <= t_exit, and THE MESH IS CUT TO THE BOX: a face test accepts t in [t_enter, t_exit] (the whole
//            clipped range, not the span of the cell it is made in).
// INTERSECT  Woop, Benthin, Wald 2013, "Watertight ray/triangle intersection".  kz = argmax |d_k| (ties to the lowest axis), kx = (kz + 1) % 3,
//            ky = (kx + 1) % 3, swapped if d[kz] < 0.  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].  Per vertex P' = P - o,
//            Px = P'[kx] - Sx P'[kz], Py = P'[ky] - Sy P'[kz], Pz = Sz P'[kz].  U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax, every
//            product rounded on its own; if any of the three is exactly 0 all three are formed in double from the same float operands and
//            rounded to float.  One negative and one positive: a miss.  det = (U + V) + W, det == 0: a miss.  T = (U Az + V Bz) + W Cz,
//            t = T / det (a t that is not finite: a miss).  No back-face culling; front = det > 0, which is the side (b - a) x (c - a) points to
//            (the shear has a positive determinant).  u = V / det (b's weight), v = W / det (c's).
// FIRST HIT  the smallest t over the valid faces, ties to the lowest face index.  Independent of the grid, its resolution and the order of a
//            cell's list; G = 1 (one cell with every valid face that touches the box) is the brute-force statement of the rule.
// GRID       G^3 cells, 1 <= G <= 128, over the box aabb = {lo, hi}; cell (ix, iy, iz) has index ix + G (iy + G iz).  The grid coordinate of x
//            on an axis is g = ((x - lo) / (hi - lo)) * G (quotient, then product, each rounded).  A valid face is listed in the cells
//            [floor(g_min - 2^-10), floor(g_max + 2^-10)] per axis, clamped to [0, G - 1]; a face whose range misses [0, G - 1] on an axis
//            (wholly outside the box) is listed nowhere.  The pad of 2^-10 of a cell is 75 x the fp32 error of o + t d at box scale.
// TRAVERSAL  Amanatides & Woo 1987 with integer cell steps from the cell of o + t_enter d (clamped into the grid).  The parameter of a cell
//            wall is recomputed from the integer index each step, ((lo + k * (hi - lo) / G) - o) / d, never accumulated.  In a cell every
//            listed face is tested; the walk stops when the parameter at which the ray leaves the cell exceeds the best t or t_exit, or when
//            the step leaves the grid.  n_tests counts the face tests (for measurement: it depends on G and on nothing else).
#pragma once
#include "meshsdf_math.hpp"
#include "ray_math.hpp"

namespace lab4d_mray {
namespace msdf = lab4d_msdf;
using lab4d_ray::point_at;
using lab4d_rn::add_rn;
using lab4d_rn::dadd;
using lab4d_rn::div_rn;
using lab4d_rn::dmul;
using lab4d_rn::finite_f;
using lab4d_rn::mul_rn;

constexpr int kMaxG = 128;
constexpr int kBlock = 256;               // lanes (rays, faces) per workgroup
constexpr int kScanBlock = 1024;          // cells per block of the offsets scan
constexpr float kPad = 0.0009765625f;     // 2^-10 of a cell
constexpr int kTriFloats = 12;            // a packed face

struct alignas(16) Quad {
  float x, y, z, w;
};

struct Hit {
  float t, u, v;
  int32_t face, front, n_tests;
};

LAB4D_HD float sel3(float x, float y, float z, int k) { return k == 0 ? x : (k == 1 ? y : z); }

// ---- packing and binning -----------------------------------------------------------------------------------------------------------------
// face f of the mesh -> its three words; returns VALID
LAB4D_HD bool pack_face(const float* verts, const int32_t* faces, int n_verts, long f, Quad* rec) {
  float v[9];
  const bool ok = msdf::load_tri(verts, faces, n_verts, f, v);
  rec[0] = Quad{v[0], v[1], v[2], ok ? 1.f : 0.f};
  rec[1] = Quad{v[3], v[4], v[5], 0.f};
  rec[2] = Quad{v[6], v[7], v[8], 0.f};
  return ok;
}

// the three words of packed face f; I is the width of the index arithmetic (the ray caster's is 64-bit)
template <class I>
LAB4D_HD void load_face(const Quad* rec, I f, Quad& a, Quad& b, Quad& c) {
  a = rec[3 * f], b = rec[3 * f + 1], c = rec[3 * f + 2];
}

// grid coordinate of x on one axis
LAB4D_HD float grid_coord(float x, float lo, float ext, int G) { return mul_rn(div_rn(x - lo, ext), (float)G); }

// the cell of x on one axis: the grid coordinate's floor, clamped into the grid (a NaN coordinate -- a box without extent -- gives cell 0)
LAB4D_HD int cell_of(float x, float lo, float ext, int G) {
  const float g = floorf(grid_coord(x, lo, ext, G));
  return g > 0.f ? (g < (float)(G - 1) ? (int)g : G - 1) : 0;
}

// the grid plane k (0 .. G) of an axis, from the integer index
LAB4D_HD float plane_at(int k, float lo, float ext, int G) { return add_rn(lo, mul_rn(div_rn((float)k, (float)G), ext)); }

// The cells of a packed face: false when it is listed nowhere (invalid, a box without extent, wholly outside); else i0[a] <= i1[a] in [0, G)
LAB4D_HD bool face_cells(const Quad* rec, const float* aabb, int G, int* i0, int* i1) {
  if (rec[0].w == 0.f) return false;
  const float pa[3] = {rec[0].x, rec[0].y, rec[0].z}, pb[3] = {rec[1].x, rec[1].y, rec[1].z}, pc[3] = {rec[2].x, rec[2].y, rec[2].z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ext = aabb[3 + a] - aabb[a];
    if (!(finite_f(aabb[a]) && finite_f(ext) && ext > 0.f)) return false;
    const float mn = fminf(pa[a], fminf(pb[a], pc[a])), mx = fmaxf(pa[a], fmaxf(pb[a], pc[a]));
    const float g0 = floorf(grid_coord(mn, aabb[a], ext, G) - kPad), g1 = floorf(grid_coord(mx, aabb[a], ext, G) + kPad);
    if (!(g1 >= 0.f && g0 <= (float)(G - 1))) return false;  // (also a NaN coordinate: an overflow of x - lo)
    i0[a] = g0 > 0.f ? (int)g0 : 0;
    i1[a] = g1 < (float)(G - 1) ? (int)g1 : G - 1;
  }
  return true;
}

// ---- the ray -------------------------------------------------------------------------------------------------------------------------------
// REJECT and CLIP: ray_math.hpp's clip_ray (0 = rejected, 1 = the clip is empty: a MISS, 2 = t_enter <= t_exit) without |d|, which the cast does not use
LAB4D_HD int clip_ray(const float* o, const float* d, float t0, float t1, const float* aabb, float* t_enter, float* t_exit) {
  float len;
  return lab4d_ray::clip_ray(o, d, t0, t1, aabb, t_enter, t_exit, &len);
}

// the shear of INTERSECT, once per ray
struct Shear {
  int kx, ky, kz;
  float Sx, Sy, Sz;
};

LAB4D_HD Shear make_shear(const float* d) {
  Shear s;
  s.kz = 0;
  if (fabsf(d[1]) > fabsf(d[0])) s.kz = 1;
  if (fabsf(d[2]) > fabsf(sel3(d[0], d[1], d[2], s.kz))) s.kz = 2;
  s.kx = s.kz == 2 ? 0 : s.kz + 1;
  s.ky = s.kx == 2 ? 0 : s.kx + 1;
  const float dz = sel3(d[0], d[1], d[2], s.kz);
  if (dz < 0.f) {
    const int k = s.kx;
    s.kx = s.ky, s.ky = k;
  }
  s.Sx = div_rn(sel3(d[0], d[1], d[2], s.kx), dz);
  s.Sy = div_rn(sel3(d[0], d[1], d[2], s.ky), dz);
  s.Sz = div_rn(1.f, dz);
  return s;
}

LAB4D_HD float edge_f(float ax, float by, float ay, float bx) { return mul_rn(ax, by) - mul_rn(ay, bx); }
LAB4D_HD float edge_d(float ax, float by, float ay, float bx) {
  return (float)dadd(dmul((double)ax, (double)by), -dmul((double)ay, (double)bx));  // (both products are exact in double)
}

// One face against one ray: true for a hit with t_lo <= t <= t_hi; then *t, *u, *v, *front are set.
LAB4D_HD bool intersect(const float* o, const Shear& s, float t_lo, float t_hi, const Quad& a, const Quad& b, const Quad& c, float* t, float* u, float* v,
                        int32_t* front) {
  const float ax = a.x - o[0], ay = a.y - o[1], az = a.z - o[2];
  const float bx = b.x - o[0], by = b.y - o[1], bz = b.z - o[2];
  const float cx = c.x - o[0], cy = c.y - o[1], cz = c.z - o[2];
  const float akz = sel3(ax, ay, az, s.kz), bkz = sel3(bx, by, bz, s.kz), ckz = sel3(cx, cy, cz, s.kz);
  const float Ax = sel3(ax, ay, az, s.kx) - mul_rn(s.Sx, akz), Ay = sel3(ax, ay, az, s.ky) - mul_rn(s.Sy, akz);
  const float Bx = sel3(bx, by, bz, s.kx) - mul_rn(s.Sx, bkz), By = sel3(bx, by, bz, s.ky) - mul_rn(s.Sy, bkz);
  const float Cx = sel3(cx, cy, cz, s.kx) - mul_rn(s.Sx, ckz), Cy = sel3(cx, cy, cz, s.ky) - mul_rn(s.Sy, ckz);
  float U = edge_f(Cx, By, Cy, Bx), V = edge_f(Ax, Cy, Ay, Cx), W = edge_f(Bx, Ay, By, Ax);
  if (U == 0.f || V == 0.f || W == 0.f) U = edge_d(Cx, By, Cy, Bx), V = edge_d(Ax, Cy, Ay, Cx), W = edge_d(Bx, Ay, By, Ax);
  if ((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f)) return false;
  const float det = add_rn(add_rn(U, V), W);
  if (det == 0.f) return false;
  const float T = add_rn(add_rn(mul_rn(U, mul_rn(s.Sz, akz)), mul_rn(V, mul_rn(s.Sz, bkz))), mul_rn(W, mul_rn(s.Sz, ckz)));
  const float tt = div_rn(T, det);
  if (!(tt >= t_lo && tt <= t_hi)) return false;  // (a NaN or infinite quotient falls out here)
  *t = tt, *u = div_rn(V, det), *v = div_rn(W, det), *front = det > 0.f ? 1 : 0;
  return true;
}

// the parameter at which the ray crosses the grid plane k (0 .. G) of an axis
LAB4D_HD float wall_t(int k, float lo, float ext, int G, float o, float d) { return div_rn(plane_at(k, lo, ext, G) - o, d); }

// One ray against the grid.  tris: n_faces packed faces; cell_start (G^3 + 1), cell_list: the lists.  Every member of the result is set.
LAB4D_HD Hit cast_ray(const float* o, const float* d, float t0, float t1, const float* aabb, int G, const float* tris, int n_faces, const int32_t* cell_start,
                      const int32_t* cell_list) {
  Hit h;
  h.t = t0, h.u = 0.f, h.v = 0.f, h.face = -1, h.front = 0, h.n_tests = 0;
  float t_enter, t_exit, p[3];
  if (n_faces == 0 || clip_ray(o, d, t0, t1, aabb, &t_enter, &t_exit) != 2) return h;
  point_at(o, d, t_enter, p);
  const Shear s = make_shear(d);
  const Quad* rec = (const Quad*)tris;
  int c[3], step[3];
  float next[3];  // the parameter at which the ray leaves the current cell along each axis (+inf on an axis it never leaves)
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ext = aabb[3 + a] - aabb[a];
    c[a] = cell_of(p[a], aabb[a], ext, G);
    step[a] = d[a] > 0.f ? 1 : (d[a] < 0.f ? -1 : 0);
    next[a] = lab4d_rn::inf_f();
    if (step[a] != 0) {
      const float w = wall_t(c[a] + (step[a] > 0 ? 1 : 0), aabb[a], ext, G, o[a], d[a]);
      if (w == w) next[a] = w;  // (0 / d with a d that underflows the quotient: NaN stays out)
    }
  }
  float best = t_exit;  // a face test accepts t <= best: nothing behind the best hit, nothing behind the exit
  for (;;) {
    const long cell = c[0] + (long)G * (c[1] + (long)G * c[2]);
    const int32_t lo = cell_start[cell], hi = cell_start[cell + 1];
    for (int32_t j = lo; j < hi; ++j) {
      const int32_t f = cell_list[j];
      Quad qa, qb, qc;
      load_face(rec, (long)f, qa, qb, qc);
      float t, u, v;
      int32_t front;
      ++h.n_tests;
      if (intersect(o, s, t_enter, best, qa, qb, qc, &t, &u, &v, &front) && (h.face < 0 || t < best || f < h.face))
        best = t, h.t = t, h.u = u, h.v = v, h.face = f, h.front = front;
    }
    const int axis = next[0] <= next[1] ? (next[0] <= next[2] ? 0 : 2) : (next[1] <= next[2] ? 1 : 2);
    const float t_leave = sel3(next[0], next[1], next[2], axis);
    if (!(t_leave <= best)) break;  // (best <= t_exit; also every axis at +inf)
    bool out = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (a == axis) {
        c[a] += step[a];
        out = c[a] < 0 || c[a] >= G;
        const float w = wall_t(c[a] + (step[a] > 0 ? 1 : 0), aabb[a], aabb[3 + a] - aabb[a], G, o[a], d[a]);
        next[a] = w == w ? w : lab4d_rn::inf_f();
      }
    if (out) break;
  }
  return h;
}

}  // namespace lab4d_mray
