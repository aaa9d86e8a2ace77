// The primitives of the kernel / CPU-twin contract, defined once.  A kernel's arithmetic lives in a csrc/*_math.hpp header behind LAB4D_HD;
// hipcc compiles it into the kernels, g++ compiles the same text into a serial twin under tests/host_harness/ (-ffp-contract=off), and the
// GPU suite holds the kernels to that twin bit for bit.  That only works if a product, sum, quotient or root that the definition rounds on
// its own is rounded on its own on BOTH sides; the functions of lab4d_rn are how the headers say so.  Plain C++ (math.h and stdint.h, no HIP
// include): g++ compiles this file alone.
//
// Why each form is what it is:
//   add_rn / mul_rn, dadd / dmul (fp32 / fp64)
//     DEVICE  HIP compiles with -ffp-contract=fast, and the backend contracts even __fmul_rn / __fadd_rn into an fma (found on the first
//             hardware run of the hash grid, see cell_of in hashgrid_math.hpp).  So the result passes through an empty asm with a "+v" operand:
//             a value the optimiser cannot see through, hence cannot fuse, at the cost of no instruction.
//     HOST    the result is stored to a volatile, which the compiler must form as written.  The harness passes -ffp-contract=off as well; the
//             volatile keeps a twin right that is built without it.
//   div_rn    __fdiv_rn on the device (the correctly rounded division whatever the fast-math flags), a volatile a / b on the host.
//   sqrt_rn   through the IEEE double root on both sides: the double root of a float, rounded once more to fp32, IS the correctly rounded
//             float root (53 >= 2 * 24 + 2 bits), and it does not depend on how a compiler's flags treat the fp32 sqrt.
//   finite_f  |v| <= FLT_MAX: false for inf and NaN.  inf_f / nan_f: the compiler's own constants, the same bits on both sides.
//   pin       the bare "+v" pin for a value that is not a fresh result (hashsdf_math.hpp: where a level's results stay, which point is
//             recomputed from); nothing on the host.
#pragma once
#include <math.h>
#include <stdint.h>

// __host__ __device__ under hipcc, nothing otherwise: what lets g++ compile a *_math.hpp header
#if defined(__HIPCC__)
#define LAB4D_HD __host__ __device__ inline
#else
#define LAB4D_HD inline
#endif

namespace lab4d_rn {

#if defined(__HIP_DEVICE_COMPILE__)
template <typename T>
__device__ __forceinline__ void pin(T& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ float add_rn(float a, float b) { float p = a + b; asm volatile("" : "+v"(p)); return p; }
__device__ __forceinline__ float mul_rn(float a, float b) { float p = a * b; asm volatile("" : "+v"(p)); return p; }
__device__ __forceinline__ float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ double dadd(double a, double b) { double p = a + b; asm volatile("" : "+v"(p)); return p; }
__device__ __forceinline__ double dmul(double a, double b) { double p = a * b; asm volatile("" : "+v"(p)); return p; }
#else  // (LAB4D_HD, not a bare inline: hipcc's host pass takes this branch too, and a __device__ caller must still resolve the call there)
template <typename T>
LAB4D_HD void pin(T&) {}
LAB4D_HD float add_rn(float a, float b) { volatile float p = a + b; return p; }
LAB4D_HD float mul_rn(float a, float b) { volatile float p = a * b; return p; }
LAB4D_HD float div_rn(float a, float b) { volatile float p = a / b; return p; }
LAB4D_HD double dadd(double a, double b) { volatile double p = a + b; return p; }
LAB4D_HD double dmul(double a, double b) { volatile double p = a * b; return p; }
#endif

LAB4D_HD float sqrt_rn(float a) { return (float)sqrt((double)a); }
LAB4D_HD bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for inf and NaN
LAB4D_HD float inf_f() { return __builtin_huge_valf(); }
LAB4D_HD float nan_f() { return __builtin_nanf(""); }

}  // namespace lab4d_rn
