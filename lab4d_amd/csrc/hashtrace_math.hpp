// Sphere tracing of the hash field's SDF to one surface hit per ray (csrc/hashtrace.hip; contract: include/lab4d_hashtrace.h).  Plain C++
// (LAB4D_HD convention) on top of hashsdf_math.hpp (the table gather), occgrid_math.hpp (to_x01, the rounded arithmetic) and ray_math.hpp
// (dir_length, point_at, clip_ray: the one statement of RAY, REJECT and CLIP): the kernel and the CPU twin
// tests/host_harness/hashtrace/hashtrace_host.cpp call the same functions.  The reference has no hash field and no tracer, so the rules are this
// repository's own; the method is Hart 1996, "Sphere tracing", with a sign-change fallback for a field that is an SDF only approximately.
//
// RAY        o + t * d, t in [t0, t1], d of any length; len = |d| as ray_math.hpp rounds it (dir_length).  eps > 0: the hit threshold on
//            |sdf| in world units; 0 < step_scale <= 1; min_step > 0: a metric length in world units; 1 <= max_steps <= 1024;
//            0 <= n_bisect <= 32.
// REJECT     a non-finite o, d, t0 or t1, t0 > t1, len == 0, or a box without extent: status MISS, t_hit = t0, n_eval = 0, sdf_hit = 0.
// CLIP       ray_math.hpp's clip_ray cuts [t0, t1] to the box (the slab test in x01 space; a parallel axis is always or never satisfied, no inf or
//            NaN arithmetic).  An empty clip is handled like a rejected ray: the tracer asks for code 2 alone, so the order of clip_ray's checks
//            does not show here.  Otherwise t_enter <= t_exit.
// EVAL       p = o + t * d (product and sum rounded on their own: point_at), x01 = (p - lo) / (hi - lo) (to_x01) CLAMPED to [0, 1] per axis
//            (rounding may push an end point out of the box; the constant sdf outside the box is never traced), s = the fused evaluator's sdf
//            at x01: gather_enc of hashsdf_math.hpp, then hidden_sdf below -- hidden() without v and without the mask.
// LOOP       t = t_enter, evaluate.  (1) the FIRST s <= 0: STARTS_INSIDE.  (2) |s| <= eps: CONVERGED.  (3) s < -eps (the previous value was
//            positive): bisect [t_prev, t] at most n_bisect times, one evaluation at the midpoint lo + 0.5 (hi - lo) each, the end with the
//            positive value stays the lower one, stop early at |s_mid| <= eps: BRACKETED, t_hit = the last midpoint evaluated (n_bisect ==
//            0: t itself).  (4) otherwise step: t == t_exit already: MISS at t_exit; t_next = t + max(step_scale * s, min_step) / len
//            (product, quotient and sum rounded on their own), cut to t_exit, so that the last evaluation sits on the exit face; t_next <= t
//            after rounding: OUT_OF_STEPS.  After max_steps evaluations of this loop: OUT_OF_STEPS.  In every case t_hit is the parameter of
//            the LAST evaluation and sdf_hit its value; n_eval <= max_steps + n_bisect; t never runs backwards outside a bisection.
//
// The walk is ONE loop with ONE evaluation per trip, whatever the lane is doing (stepping or bisecting): on the device the lanes of a wave
// that are in different phases still share the gather and the net, and the evaluator is inlined once.
#pragma once
#include "hashsdf_math.hpp"
#include "occgrid_math.hpp"
#include "ray_math.hpp"

namespace lab4d_trace {
namespace hs = lab4d_hsdf;
namespace occ = lab4d_occ;
namespace ray = lab4d_ray;
using lab4d_rn::add_rn;
using lab4d_rn::div_rn;
using lab4d_rn::finite_f;
using lab4d_rn::mul_rn;

constexpr int kMiss = 0, kConverged = 1, kBracketed = 2, kStartsInside = 3, kOutOfSteps = 4;
constexpr int kMaxSteps = 1024, kMaxBisect = 32;
constexpr int kBlock = 256;  // lanes (rays) per workgroup

struct Params {
  float eps, step_scale, min_step;
  int max_steps, n_bisect;
};

LAB4D_HD bool params_ok(const Params& q) {
  return finite_f(q.eps) && q.eps > 0.f && q.step_scale > 0.f && q.step_scale <= 1.f && finite_f(q.min_step) && q.min_step > 0.f && q.max_steps >= 1 &&
         q.max_steps <= kMaxSteps && q.n_bisect >= 0 && q.n_bisect <= kMaxBisect;
}

struct Hit {
  float t, sdf;
  int status, n_eval;
};

// the sdf of hidden() (hashsdf_math.hpp) alone: z row by row, neither v = W1^T (m * w2) nor the mask word
LAB4D_HD float hidden_sdf(const float* enc, const float* W1, const float* b1, const float* w2, float b2) {
  float sdf = b2;
#pragma unroll 2  // (as hidden(): fully unrolled, the 2,048 LDS reads are hoisted into registers)
  for (int j = 0; j < hs::kHid; ++j) {
    const float* row = W1 + j * hs::kEnc;
    float z = b1[j];
#pragma unroll
    for (int k = 0; k < hs::kEnc; ++k) z += row[k] * enc[k];
    const float q = z > 0.f ? w2[j] : 0.f;
    sdf += q * z;
  }
  return sdf;
}

// the field's sdf at box coordinates x01 in [0,1]^3
template <int F>
LAB4D_HD float sdf_at(const float* x01, const float* table, const int* res, int log2_T, const float* W1, const float* b1, const float* w2, float b2) {
  float enc[hs::kEnc];
  hs::gather_enc<F>(x01, table, res, log2_T, 0.f, nullptr, enc, nullptr);
  return hidden_sdf(enc, W1, b1, w2, b2);
}

// REJECT and CLIP as the tracer asks them of ray_math.hpp's clip_ray: true iff the ray enters the loop; then *t_enter <= *t_exit and *len = |d| > 0
LAB4D_HD bool clip_ray(const float* o, const float* d, float t0, float t1, const float* aabb, float* t_enter, float* t_exit, float* len) {
  return ray::clip_ray(o, d, t0, t1, aabb, t_enter, t_exit, len) == 2;
}

// x01 of the ray's point at t, clamped into the box
LAB4D_HD void x01_at(const float* o, const float* d, float t, const float* aabb, float* x01) {
  float p[3];
  ray::point_at(o, d, t, p);
#pragma unroll
  for (int a = 0; a < 3; ++a) x01[a] = fminf(fmaxf(occ::to_x01(p[a], aabb[a], aabb[3 + a]), 0.f), 1.f);
}

LAB4D_HD float midpoint(float lo, float hi) { return add_rn(lo, mul_rn(0.5f, hi - lo)); }

// One ray.  eval(x01) -> sdf is the field (sdf_at with the caller's pointers).  Every member of the result is set.
template <class Eval>
LAB4D_HD Hit trace_ray(const float* o, const float* d, float t0, float t1, const float* aabb, const Params& q, Eval&& eval) {
  Hit h;
  h.t = t0, h.sdf = 0.f, h.status = kMiss, h.n_eval = 0;
  float t, t_exit, len;
  if (!clip_ray(o, d, t0, t1, aabb, &t, &t_exit, &len)) return h;
  float lo = t, hi = t;  // the bracket: sdf(lo) > eps, and once a bisection runs sdf(hi) < -eps
  int n_main = 0, n_bis = -1;  // n_bis < 0: stepping
  for (;;) {
    float x01[3];
    x01_at(o, d, t, aabb, x01);
    const float s = eval(x01);
    ++h.n_eval;
    h.t = t, h.sdf = s;
    if (n_bis < 0) {
      ++n_main;
      if (n_main == 1 && s <= 0.f) { h.status = kStartsInside; break; }
      if (fabsf(s) <= q.eps) { h.status = kConverged; break; }
      if (s < 0.f) {  // below -eps, and the previous value was above eps
        h.status = kBracketed;
        if (q.n_bisect == 0) break;
        hi = t, n_bis = 0;
        t = midpoint(lo, hi);
        continue;
      }
      if (t == t_exit) break;  // (MISS)
      h.status = kOutOfSteps;
      float t_next = add_rn(t, div_rn(fmaxf(mul_rn(q.step_scale, s), q.min_step), len));
      if (t_next > t_exit) t_next = t_exit;
      if (!(t_next > t) || n_main == q.max_steps) break;
      h.status = kMiss;
      lo = t, t = t_next;
    } else {
      ++n_bis;
      if (fabsf(s) <= q.eps || n_bis == q.n_bisect) break;  // (BRACKETED)
      if (s > 0.f) lo = t; else hi = t;
      t = midpoint(lo, hi);
    }
  }
  return h;
}

}  // namespace lab4d_trace
