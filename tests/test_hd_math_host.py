"""lab4d_amd/csrc/hd_math.hpp on the CPU: the rounded primitives that every kernel / twin pair is built from (tests/host_harness/hd_math_host.cpp)
against numpy, bit for bit.  numpy's float32 + * / sqrt and float64 + * are the correctly rounded IEEE operations, np.isfinite is the definition of
finite_f.  Bit patterns are compared (uint32 / uint64 views); a NaN matches any NaN.  CPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402

F32_EDGES = np.array([0x00000000, 0x80000000,   # +-0
                      0x00000001, 0x80000001,   # smallest denormal
                      0x007fffff, 0x807fffff,   # largest denormal
                      0x00800000, 0x80800000,   # FLT_MIN
                      0x7f7fffff, 0xff7fffff,   # FLT_MAX
                      0x7f800000, 0xff800000,   # inf
                      0x7fc00000, 0xffc00001,   # NaN
                      0x3f800000, 0xbf800000, 0x40000000, 0x3f000000], np.uint32).view(np.float32)  # +-1, 2, 0.5
F64_EDGES = np.array([0.0, -0.0, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308, np.inf, -np.inf, np.nan, 1.0, -1.0,
                      2.0, 0.5], np.float64)


def _pairs(edges, rand_a, rand_b):
    """every edge value against every edge value (FLT_MAX + FLT_MAX, FLT_MAX * 2, inf - inf, 0 / 0, ... are among them), every edge against a random
    value from both sides, and the random pairs"""
    k = edges.size
    ea, eb = np.repeat(edges, k), np.tile(edges, k)
    a = np.concatenate([ea, edges, rand_b[:k], rand_a])
    b = np.concatenate([eb, rand_a[:k], edges, rand_b])
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


@pytest.fixture(scope="module")
def host():
    return host_twin.load("hd_math")


@pytest.fixture(scope="module")
def f32_pairs():
    rng = np.random.default_rng(20240)
    ra, rb = (rng.integers(0, 1 << 32, 10000, dtype=np.uint32).view(np.float32) for _ in range(2))
    return _pairs(F32_EDGES, ra, rb)


@pytest.fixture(scope="module")
def f64_pairs():
    rng = np.random.default_rng(20241)
    ra, rb = (rng.integers(0, 1 << 64, 10000, dtype=np.uint64).view(np.float64) for _ in range(2))
    return _pairs(F64_EDGES, ra, rb)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _run(fn, *inputs, out_dtype=None):
    out = np.empty(inputs[0].size, out_dtype or inputs[0].dtype)
    fn(*[_ptr(x) for x in inputs], inputs[0].size, _ptr(out))
    return out


def _assert_same_bits(got, want):
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    assert got.dtype == want.dtype
    same = (got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("name, op", [("add", np.add), ("mul", np.multiply), ("div", np.divide)])
def test_fp32_binary_is_the_correctly_rounded_operation(host, f32_pairs, name, op):
    a, b = f32_pairs
    with np.errstate(all="ignore"):
        want = op(a, b)
    _assert_same_bits(_run(getattr(host, "hd_math_host_" + name), a, b), want)


def test_sqrt_rn_is_the_correctly_rounded_root(host, f32_pairs):
    a = f32_pairs[0]
    with np.errstate(all="ignore"):
        want = np.sqrt(a)  # negative: NaN; -0: -0
    _assert_same_bits(_run(host.hd_math_host_sqrt, a), want)


def test_finite_f_is_isfinite(host, f32_pairs):
    a = f32_pairs[0]
    assert np.array_equal(_run(host.hd_math_host_finite, a, out_dtype=np.uint8), np.isfinite(a).astype(np.uint8))


@pytest.mark.parametrize("name, op", [("dadd", np.add), ("dmul", np.multiply)])
def test_fp64_binary_is_the_correctly_rounded_operation(host, f64_pairs, name, op):
    a, b = f64_pairs
    with np.errstate(all="ignore"):
        want = op(a, b)
    _assert_same_bits(_run(getattr(host, "hd_math_host_" + name), a, b), want)


def test_product_is_rounded_before_the_sum(host):
    """a = b = 1 + 2^-12, c = -(1 + 2^-11): a * b = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 (half an ulp, to even), so the two-step result is exactly
    0; a fused multiply-add would keep the 2^-24.  The same one precision up: 1 + 2^-27 and -(1 + 2^-26), where 2^-54 is a quarter of an ulp."""
    a = np.array([1 + 2.0 ** -12], np.float32)
    c = np.array([-(1 + 2.0 ** -11)], np.float32)
    assert float(a[0]) * float(a[0]) + float(c[0]) == 2.0 ** -24  # (exact in float64: what a fused evaluation returns)
    got = _run(host.hd_math_host_mul_add, a, a, c)
    assert got.view(np.uint32)[0] == 0, got
    ad = np.array([1 + 2.0 ** -27], np.float64)
    cd = np.array([-(1 + 2.0 ** -26)], np.float64)
    got = _run(host.hd_math_host_dmul_add, ad, ad, cd)
    assert got.view(np.uint64)[0] == 0, got


def test_constants_and_the_host_pin(host, f32_pairs):
    out = np.zeros(2, np.float32)
    host.hd_math_host_constants(_ptr(out))
    assert out.view(np.uint32)[0] == 0x7f800000 and np.isnan(out[1])
    a = f32_pairs[0]
    assert np.array_equal(_run(host.hd_math_host_pin, a).view(np.uint32), a.view(np.uint32))  # nothing on the host: NaN payloads included
