// CPU twin of lab4d_amd/csrc/hashtrace.hip: a serial loop over the SAME functions (csrc/hashtrace_math.hpp) with the layout and the argument
// checks of include/lab4d_hashtrace.h.  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_hashtrace_host.py holds it to a
// float64 root search over oracle/hashgrid_oracle.py.  Returns 0, or -1 for arguments outside the contract.  A folder of its own: the census of
// tests/test_host_twin.py counts the twins beside it.
#include <stdint.h>

#include "hashtrace_math.hpp"

namespace tr = lab4d_trace;

template <int F>
static void trace_t(const float* origin, const float* dir, const float* t_range, const float* aabb, long R, const float* table, const int32_t* res,
                    int log2_T, const float* W1, const float* b1, const float* w2, const float* b2, const tr::Params& q, float* t_hit, int32_t* status,
                    int32_t* n_eval, float* sdf_hit) {
  for (long r = 0; r < R; ++r) {
    const tr::Hit h = tr::trace_ray(origin + 3 * r, dir + 3 * r, t_range[2 * r], t_range[2 * r + 1], aabb, q,
                                    [&](const float* x01) { return tr::sdf_at<F>(x01, table, res, log2_T, W1, b1, w2, b2[0]); });
    t_hit[r] = h.t, status[r] = h.status, n_eval[r] = h.n_eval, sdf_hit[r] = h.sdf;
  }
}

// REJECT and CLIP alone: ok (R) uint8 = the ray enters the loop, t_clip (R,2) = {t_enter, t_exit} (t0, t0 for a ray that does not)
extern "C" void hashtrace_host_clip(const float* origin, const float* dir, const float* t_range, const float* aabb, long R, float* t_clip, uint8_t* ok) {
  for (long r = 0; r < R; ++r) {
    float len;
    t_clip[2 * r] = t_clip[2 * r + 1] = t_range[2 * r];
    ok[r] = tr::clip_ray(origin + 3 * r, dir + 3 * r, t_range[2 * r], t_range[2 * r + 1], aabb, t_clip + 2 * r, t_clip + 2 * r + 1, &len) ? 1 : 0;
  }
}

extern "C" int hashtrace_host_trace(const float* origin, const float* dir, const float* t_range, const float* aabb, long R, const float* table,
                                    const int32_t* res, int L, int log2_T, int F, const float* W1, const float* b1, const float* w2, const float* b2,
                                    float eps, float step_scale, float min_step, int max_steps, int n_bisect, float* t_hit, int32_t* status,
                                    int32_t* n_eval, float* sdf_hit) {
  const tr::Params q = {eps, step_scale, min_step, max_steps, n_bisect};
  if (R < 0 || L < 1 || L > 32 || F < 1 || F > 8 || L * F != lab4d_hsdf::kEnc || log2_T < 4 || log2_T > 24 || !tr::params_ok(q)) return -1;
  if (R == 0) return 0;
  if (F == 1) trace_t<1>(origin, dir, t_range, aabb, R, table, res, log2_T, W1, b1, w2, b2, q, t_hit, status, n_eval, sdf_hit);
  else if (F == 2) trace_t<2>(origin, dir, t_range, aabb, R, table, res, log2_T, W1, b1, w2, b2, q, t_hit, status, n_eval, sdf_hit);
  else if (F == 4) trace_t<4>(origin, dir, t_range, aabb, R, table, res, log2_T, W1, b1, w2, b2, q, t_hit, status, n_eval, sdf_hit);
  else trace_t<8>(origin, dir, t_range, aabb, R, table, res, log2_T, W1, b1, w2, b2, q, t_hit, status, n_eval, sdf_hit);
  return 0;
}
