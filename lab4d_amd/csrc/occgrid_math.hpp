// Occupancy bit grid of the hash field (csrc/occgrid.hip; contract: include/lab4d_occgrid.h): a bit per cell of a coarse grid over the
// field's box, refreshed from the field's own density, consulted per sample (skip empty cells) and per ray (march only between the first
// and the last occupied cell) -- Mueller et al. 2022, section 5.4 / appendix E.  The reference has no counterpart (nnutils/nerf.py:98 is
// a TODO), so the rules below are this repository's own.
// Plain C++ behind LAB4D_HD (see hd_math.hpp): the kernels run these functions one lane per cell / sample / ray,
// tests/host_harness/occgrid_host.cpp compiles them with g++ (-ffp-contract=off) as serial loops, and the GPU suite holds the kernels
// bit for bit to that twin.  Every product that feeds a sum or a comparison is rounded on its own (mul_rn / add_rn, see hd_math.hpp);
// 1 / d is the correctly rounded division on both sides.
//
// GRID   G cells per axis over aabb = {lo, hi}, 2 <= G <= 256.  x01 = (x - lo) / (hi - lo) per axis (the arithmetic of
//        hashfield.forward).  A point has a cell iff 0 <= x01 <= 1 on every axis (NaN: no cell; an empty box hi <= lo: no point has one);
//        its cell along an axis is min(G - 1, int(x01 * G)), so that x01 == 1 lies in the last cell and a point ON an inner cell face
//        belongs to the cell of the HIGHER index.  Linear index (i * G + j) * G + k, x slowest (proxy.sample_grid's order); cell idx is
//        bit (idx & 31) of 32-bit word (idx >> 5); ceil(G^3 / 32) words, the unused bits of the last word are zero.
// UPDATE ema_new = max(ema_old * decay, d) with d the cell's fresh density (NaN or negative: 0); bit = ema_new > thresh.  A new grid has
//        every bit set and ema = +inf ("nothing known yet"); the first update of such a cell replaces it: ema_new = d.
// MASK   mask[s] = 1 iff the point has a cell and the cell's bit is set.
// SPAN   ray o + t * d, t in [t0, t1], d of any length (t is in the caller's own depth units).  In x01 space o01 = (o - lo) / (hi - lo),
//        d01 = d / (hi - lo).  The ray is clipped to [0,1]^3 with the slab test; an axis whose d01 is zero (or so small that 1 / d01 is
//        not finite) is PARALLEL: its slab is always satisfied when 0 <= o01 <= 1 and never otherwise, and the walk never steps along it.
//        A ray with a non-finite input, t0 > t1 or an empty box misses.  The cells are then walked in order (Amanatides & Woo 1987) from
//        the cell of the clipped entry point (coordinates clamped into the grid), at most 3 * G cells: the exit parameter of the current
//        cell on axis a is ((c[a] + (d01[a] > 0)) / G - o01[a]) * (1 / d01[a]), formed from the cell index every time (nothing
//        accumulates), the cell is left through the axis with the smallest exit parameter, and the parameter never runs backwards.
//        TIES: when two or three axes share the smallest exit parameter (the ray goes through a cell edge or corner) ONE axis is stepped,
//        the one with the lowest index (x before y before z); the next cell is then visited with an interval of zero length and left
//        through the next tied axis.  The rule looks at the parameters only, so it is the same for negative and positive directions; a ray
//        that starts on a face going down starts in the higher cell (the floor rule of GRID) and leaves it at once the same way.
//        t_first = entry parameter of the first occupied cell visited (>= t0), t_last = exit parameter of the last one (<= t1), hit = an
//        occupied cell was visited; hit == 0: t_first = t_last = t0.  Every visited cell counts, also one crossed in zero length, so the
//        span errs on the wide side.
#pragma once
#include "hd_math.hpp"

namespace lab4d_occ {
using lab4d_rn::add_rn;
using lab4d_rn::div_rn;
using lab4d_rn::finite_f;
using lab4d_rn::mul_rn;

constexpr int kMinG = 2, kMaxG = 256;

LAB4D_HD long n_cells(int G) { return (long)G * G * G; }
LAB4D_HD long n_words(int G) { return (n_cells(G) + 31) >> 5; }
LAB4D_HD long linear_index(int i, int j, int k, int G) { return ((long)i * G + j) * G + k; }
LAB4D_HD bool bit_of(const uint32_t* bits, long idx) { return (bits[idx >> 5] >> (idx & 31)) & 1u; }

// ---- update -------------------------------------------------------------------------------------------------------------------------
// (the product feeds a comparison, never a sum: there is nothing it could be contracted with, it is rounded as written on both sides)
LAB4D_HD float ema_next(float ema_old, float density, float decay) {
  const float d = density > 0.f ? density : 0.f;  // NaN and negative: 0
  if (ema_old > 3.402823466e+38f) return d;       // +inf: nothing known yet
  const float p = ema_old * decay;
  return p > d ? p : d;
}
LAB4D_HD bool occupied(float ema, float thresh) { return ema > thresh; }

// ---- per-sample ---------------------------------------------------------------------------------------------------------------------
LAB4D_HD float to_x01(float x, float lo, float hi) { return div_rn(x - lo, hi - lo); }

// cell along one axis of x01 in [0,1]; -1 for a coordinate outside it or NaN
LAB4D_HD int cell_axis(float x01, int G) {
  if (!(x01 >= 0.f && x01 <= 1.f)) return -1;
  const int c = (int)mul_rn(x01, (float)G);
  return c < G - 1 ? c : G - 1;
}

// linear cell index of a world point, -1 if it has none
LAB4D_HD long cell_of_point(const float* p, const float* aabb, int G) {
  int c[3];
  for (int a = 0; a < 3; ++a) {
    if (!(aabb[3 + a] - aabb[a] > 0.f)) return -1;
    c[a] = cell_axis(to_x01(p[a], aabb[a], aabb[3 + a]), G);
    if (c[a] < 0) return -1;
  }
  return linear_index(c[0], c[1], c[2], G);
}

LAB4D_HD bool sample_mask(const float* p, const float* aabb, const uint32_t* bits, int G) {
  const long idx = cell_of_point(p, aabb, G);
  return idx >= 0 && bit_of(bits, idx);
}

// ---- per-ray ------------------------------------------------------------------------------------------------------------------------
// exit parameter of cell c on an axis the ray moves along (inv = 1 / d01, up = d01 > 0)
LAB4D_HD float axis_exit(int c, bool up, int G, float o01, float inv) {
  return mul_rn(div_rn((float)(c + (up ? 1 : 0)), (float)G) - o01, inv);
}

// t_span[0] = t_first, t_span[1] = t_last; returns hit.  n_steps (may be null): cells visited, never more than 3 * G.
LAB4D_HD bool ray_span(const float* o, const float* d, float t0, float t1, const float* aabb, const uint32_t* bits, int G, float* t_span,
                       int* n_steps) {
  t_span[0] = t_span[1] = t0;
  if (n_steps) *n_steps = 0;
  if (!(finite_f(t0) && finite_f(t1) && t0 <= t1)) return false;
  float o01[3], d01[3], inv[3];
  bool moves[3], up[3];
  float tmin = t0, tmax = t1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ext = aabb[3 + a] - aabb[a];
    if (!(finite_f(o[a]) && finite_f(d[a]) && ext > 0.f)) return false;
    o01[a] = div_rn(o[a] - aabb[a], ext);
    d01[a] = div_rn(d[a], ext);
    inv[a] = d01[a] != 0.f ? div_rn(1.f, d01[a]) : 0.f;
    moves[a] = d01[a] != 0.f && finite_f(inv[a]);
    up[a] = d01[a] > 0.f;
    if (!finite_f(o01[a])) return false;
    if (!moves[a]) {
      if (!(o01[a] >= 0.f && o01[a] <= 1.f)) return false;
      continue;
    }
    const float ta = mul_rn(0.f - o01[a], inv[a]), tb = mul_rn(1.f - o01[a], inv[a]);
    const float tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
    if (tn > tmin) tmin = tn;
    if (tf < tmax) tmax = tf;
  }
  if (!(tmin <= tmax)) return false;
  int c[3];
  float ex[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float p = moves[a] ? add_rn(o01[a], mul_rn(tmin, d01[a])) : o01[a];
    const float q = mul_rn(p, (float)G);
    c[a] = q >= (float)(G - 1) ? G - 1 : (q > 0.f ? (int)q : 0);
    ex[a] = moves[a] ? axis_exit(c[a], up[a], G, o01[a], inv[a]) : 0.f;
  }
  bool hit = false;
  float t_cur = tmin;
  for (int step = 0; step < 3 * G; ++step) {
    if (n_steps) *n_steps = step + 1;
    // the moving axis with the smallest exit parameter; ties: the lowest index.  (Written without an indexed access to c / ex, so that
    // they stay in registers on the device.)
    int ax = -1;
    float t_exit = tmax;
    if (moves[2]) { ax = 2; t_exit = ex[2]; }
    if (moves[1] && (ax < 0 || ex[1] <= t_exit)) { ax = 1; t_exit = ex[1]; }
    if (moves[0] && (ax < 0 || ex[0] <= t_exit)) { ax = 0; t_exit = ex[0]; }
    if (t_exit < t_cur) t_exit = t_cur;
    if (bit_of(bits, linear_index(c[0], c[1], c[2], G))) {
      if (!hit) t_span[0] = t_cur;
      t_span[1] = t_exit < tmax ? t_exit : tmax;
      hit = true;
    }
    if (ax < 0 || !(t_exit < tmax)) break;
    bool left = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (a == ax) {
        c[a] += up[a] ? 1 : -1;
        left = c[a] < 0 || c[a] >= G;
        if (!left) ex[a] = axis_exit(c[a], up[a], G, o01[a], inv[a]);
      }
    if (left) break;
    t_cur = t_exit;
  }
  return hit;
}

}  // namespace lab4d_occ
