// A ray against a box, stated once for every kernel that casts one: the packed march (packed_math.hpp), the sphere tracer (hashtrace_math.hpp) and
// the mesh ray caster (meshray_math.hpp) and their CPU twins all call these functions.  Plain C++ behind LAB4D_HD on hd_math.hpp's individually
// rounded products, sums, quotients and roots alone.
//
// RAY     o + t * d, t in [t0, t1] in units of d, d of any length.  len = |d| = the correctly rounded root of the three rounded squares added x, then
//         y, then z (dir_length).  The point at t is o + t * d with the product and the sum rounded on their own (point_at).
// REJECT  checked FIRST, on all three axes: a non-finite t0 or t1, t0 > t1, a non-finite o, d or extent hi - lo, an extent that is not > 0, len == 0:
//         code 0.  Only then the slabs: the order decides 0 against 1 (a rejected ray that also misses the box is rejected).  An o01 that overflows
//         is rejected where its axis' slab is reached.
// CLIP    [t0, t1] is cut to the box aabb = {lo, hi} with the slab test in x01 space, o01 = (o - lo) / (hi - lo), d01 = d / (hi - lo): an axis whose d01
//         is zero or whose 1 / d01 is not finite is PARALLEL -- always satisfied when 0 <= o01 <= 1, never otherwise --, no inf or NaN arithmetic
//         occurs.  An empty clip: code 1.  Otherwise code 2 and t_enter <= t_exit.  (occgrid_math.hpp's ray_span is a different rule, not a copy: it
//         keeps o01, d01 and 1 / d01 for its walk and does not ask for a finite extent.)
#pragma once
#include "hd_math.hpp"

namespace lab4d_ray {
using lab4d_rn::add_rn;
using lab4d_rn::div_rn;
using lab4d_rn::finite_f;
using lab4d_rn::mul_rn;
using lab4d_rn::sqrt_rn;

LAB4D_HD float dir_length(const float* d) { return sqrt_rn(add_rn(add_rn(mul_rn(d[0], d[0]), mul_rn(d[1], d[1])), mul_rn(d[2], d[2]))); }

LAB4D_HD void point_at(const float* o, const float* d, float t, float* p) {
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = add_rn(o[a], mul_rn(t, d[a]));
}

// REJECT and CLIP: 0 = rejected, 1 = the clip is empty, 2 = *t_enter <= *t_exit (written for 2 alone).  *len = |d| whenever the code is not 0.
LAB4D_HD int clip_ray(const float* o, const float* d, float t0, float t1, const float* aabb, float* t_enter, float* t_exit, float* len) {
  if (!(finite_f(t0) && finite_f(t1) && t0 <= t1)) return 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ext = aabb[3 + a] - aabb[a];
    if (!(finite_f(o[a]) && finite_f(d[a]) && finite_f(ext) && ext > 0.f)) return 0;
  }
  *len = dir_length(d);
  if (!(*len > 0.f)) return 0;
  float tmin = t0, tmax = t1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float ext = aabb[3 + a] - aabb[a];
    const float o01 = div_rn(o[a] - aabb[a], ext), d01 = div_rn(d[a], ext);
    if (!finite_f(o01)) return 0;
    const float inv = d01 != 0.f ? div_rn(1.f, d01) : 0.f;
    if (!(d01 != 0.f && finite_f(inv))) {  // parallel
      if (!(o01 >= 0.f && o01 <= 1.f)) return 1;
      continue;
    }
    const float ta = mul_rn(0.f - o01, inv), tb = mul_rn(1.f - o01, inv);
    const float tn = ta < tb ? ta : tb, tf = ta < tb ? tb : ta;
    if (tn > tmin) tmin = tn;
    if (tf < tmax) tmax = tf;
  }
  if (!(tmin <= tmax)) return 1;
  *t_enter = tmin;
  *t_exit = tmax;
  return 2;
}

}  // namespace lab4d_ray
