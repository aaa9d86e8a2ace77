// The host side of lab4d_amd/csrc/hd_math.hpp on its own: array loops over the lab4d_rn functions that every CPU twin is built from.
// Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_hd_math_host.py holds each loop bit for bit to numpy.
#include "hd_math.hpp"

namespace rn = lab4d_rn;

extern "C" void hd_math_host_add(const float* a, const float* b, long n, float* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::add_rn(a[i], b[i]);
}
extern "C" void hd_math_host_mul(const float* a, const float* b, long n, float* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::mul_rn(a[i], b[i]);
}
extern "C" void hd_math_host_div(const float* a, const float* b, long n, float* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::div_rn(a[i], b[i]);
}
extern "C" void hd_math_host_sqrt(const float* a, long n, float* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::sqrt_rn(a[i]);
}
extern "C" void hd_math_host_finite(const float* a, long n, uint8_t* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::finite_f(a[i]) ? 1 : 0;
}
// out[i] = a[i] * b[i] + c[i], product and sum rounded separately
extern "C" void hd_math_host_mul_add(const float* a, const float* b, const float* c, long n, float* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::add_rn(rn::mul_rn(a[i], b[i]), c[i]);
}
extern "C" void hd_math_host_dadd(const double* a, const double* b, long n, double* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::dadd(a[i], b[i]);
}
extern "C" void hd_math_host_dmul(const double* a, const double* b, long n, double* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::dmul(a[i], b[i]);
}
extern "C" void hd_math_host_dmul_add(const double* a, const double* b, const double* c, long n, double* out) {
  for (long i = 0; i < n; ++i) out[i] = rn::dadd(rn::dmul(a[i], b[i]), c[i]);
}
// out = {inf_f(), nan_f()}; a pinned value is the value (the pin is nothing on the host)
extern "C" void hd_math_host_constants(float* out) {
  out[0] = rn::inf_f();
  out[1] = rn::nan_f();
}
extern "C" void hd_math_host_pin(const float* a, long n, float* out) {
  for (long i = 0; i < n; ++i) {
    float v = a[i];
    rn::pin(v);
    out[i] = v;
  }
}
