// Camera-visibility culling of the occupancy grids (csrc/occvis.hip; contract: include/lab4d_occvis.h): which cells of a G^3 grid does at
// least one of M camera frusta, given as six world-space half-spaces each, see.  Plain C++ behind LAB4D_HD (see hd_math.hpp): the kernel runs
// these functions one lane per cell, tests/host_harness/occvis/occvis_host.cpp compiles them with g++ (-ffp-contract=off) as serial loops,
// and the GPU suite holds the kernels word for word to that twin.  Every product and sum is rounded on its own (mul_rn / add_rn, dmul / dadd).
//
// BOX    cell i along an axis of a box [lo, hi] with G cells: in float64 e = hi - lo, h = e / (2 G), c = lo + (2 i + 1) h, then c and h
//        rounded to fp32 once each.  In fp32 the sum lo + (2 i + 1) h would lose |lo| ulps where the box straddles the origin and |c| is
//        small; no slack in terms of |c| and h covers that.  (The IEEE double quotient is the same on both sides, as the double root of
//        hd_math.hpp's sqrt_rn is; six of them per cell, against 6 M plane tests.)
// SEES   a plane {nx, ny, nz, d} keeps the box iff v = n.c + |n|.h + d >= -slack with slack = 16 * 2^-23 * (sum_a |n_a| q_a + |d|),
//        q_a = |c_a| + h_a, in the order written in plane_keeps; a view sees the box iff its 24 coefficients are finite and all six planes
//        keep it.  The derivation of the slack (4.5 * 2^-23 B is the bound on the rounding; 16 is what the rule uses) is in the header.
#pragma once
#include "occgrid_math.hpp"

namespace lab4d_occvis {
using lab4d_rn::add_rn;
using lab4d_rn::dadd;
using lab4d_rn::dmul;
using lab4d_rn::finite_f;
using lab4d_rn::mul_rn;

constexpr int kMaxM = 1 << 20, kMinK = 1, kMaxK = 8;
constexpr int kTile = 64;                  // views per LDS tile of the kernel
constexpr float kSlack = 16.f * 1.1920929e-07f;  // 16 * 2^-23 = 2^-19, exact

// centre and half extent of cell i along one axis
LAB4D_HD void cell_axis_box(float lo, float hi, int i, int G, float* c, float* h) {
  const double hh = dadd((double)hi, -(double)lo) / (double)(2 * G);
  *c = (float)dadd((double)lo, dmul((double)(2 * i + 1), hh));
  *h = (float)hh;
}

// c, h, q (3 each) of the cell with linear index idx (GRID of occgrid_math.hpp: x slowest)
LAB4D_HD void cell_box(long idx, const float* aabb, int G, float* c, float* h, float* q) {
  const int k = (int)(idx % G), j = (int)((idx / G) % G), i = (int)(idx / ((long)G * G));
  const int cell[3] = {i, j, k};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cell_axis_box(aabb[a], aabb[3 + a], cell[a], G, &c[a], &h[a]);
    q[a] = add_rn(fabsf(c[a]), h[a]);
  }
}

LAB4D_HD bool view_finite(const float* planes24) {
  bool ok = true;
  for (int e = 0; e < 24; ++e) ok = ok && finite_f(planes24[e]);
  return ok;
}

LAB4D_HD bool plane_keeps(float nx, float ny, float nz, float d, const float* c, const float* h, const float* q) {
  float v = add_rn(mul_rn(nx, c[0]), mul_rn(ny, c[1]));
  v = add_rn(v, mul_rn(nz, c[2]));
  v = add_rn(v, mul_rn(fabsf(nx), h[0]));
  v = add_rn(v, mul_rn(fabsf(ny), h[1]));
  v = add_rn(v, mul_rn(fabsf(nz), h[2]));
  v = add_rn(v, d);
  float b = add_rn(mul_rn(fabsf(nx), q[0]), mul_rn(fabsf(ny), q[1]));
  b = add_rn(b, mul_rn(fabsf(nz), q[2]));
  b = add_rn(b, fabsf(d));
  return v >= -mul_rn(kSlack, b);  // (NaN in the box: false)
}

// the six planes of one view whose coefficients are finite (view_finite is the caller's: once per view, not per cell)
LAB4D_HD bool view_sees(const float* planes24, const float* c, const float* h, const float* q) {
  bool in = true;
#pragma unroll
  for (int p = 0; p < 6; ++p) in = in & plane_keeps(planes24[4 * p], planes24[4 * p + 1], planes24[4 * p + 2], planes24[4 * p + 3], c, h, q);
  return in;
}

// APPLY per cell: the new bit; *ema is cleared where the cell is invisible
LAB4D_HD bool apply_cell(bool bit, bool vis, float* ema) {
  if (!vis) *ema = 0.f;
  return bit && vis;
}

}  // namespace lab4d_occvis
