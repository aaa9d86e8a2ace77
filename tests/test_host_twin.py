"""tests/host_twin.py: every extern "C" function of every CPU twin is typed from its source, four signatures written out by hand, and what the
parser and the typed functions refuse.  CPU only."""
import ctypes
import glob
import os
import re

import pytest

import host_twin

SOURCES = sorted(glob.glob(os.path.join(host_twin.HARNESS, "*_host.cpp")))
vp, ci, cl, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


def test_census_every_function_of_every_twin_is_typed():
    """the count of `extern "C"` in the comment-stripped text (plain, not the helper's pattern) is the number of functions load() typed -- a
    definition the pattern cannot read is not silently left with ctypes' defaults -- and each resolves in the built library"""
    total = 0
    for src in SOURCES:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(src).read(), flags=re.S)
        lib = host_twin.load(os.path.basename(src)[:-len("_host.cpp")])
        names = re.findall(r"\b(\w+)\s*\(", " ".join(chunk.split("{")[0] for chunk in text.split('extern "C"')[1:]))
        assert len(names) == text.count('extern "C"') > 0, (src, names)
        for n in names:
            assert getattr(lib, n).argtypes is not None, (src, n)  # (ctypes keeps the function object: this is the one load() typed)
        total += len(names)
    assert (len(SOURCES), total) == (11, 40)


def test_pinned_signatures():
    fn = host_twin.load("sample_pdf").row_sum_host
    assert fn.restype is cf and list(fn.argtypes) == [vp, ci, cf]
    fn = host_twin.load("mesh").mesh_host_extract
    assert fn.restype is None and list(fn.argtypes) == [vp, vp, ci, ci, ci, cf, vp, vp, vp, cl, cl, vp]
    a = list(host_twin.load("optim").adamw_host_step.argtypes)
    assert len(a) == 14 and a[4] is ctypes.c_longlong and a[7] is ci and a[12] is ci
    a = list(host_twin.load("hashsdf").hashsdf_host_backward.argtypes)
    assert len(a) == 18 and a[-1] is ci


def test_parser_refuses_types_outside_the_maps():
    with pytest.raises(TypeError, match=r"t\.cpp.*double scale.*scaled_host"):
        host_twin.signatures('extern "C" int scaled_host(const float* x, double scale) { return 0; }', "t.cpp")
    with pytest.raises(TypeError, match=r"t\.cpp.*size_t.*count_host"):
        host_twin.signatures('extern "C" size_t count_host(const float* x, int n) { return 0; }', "t.cpp")


def test_typed_functions_refuse_a_bad_call_before_the_twin_runs():
    fn = host_twin.load("packed").packed_host_march_count  # (origin, dir, t_range, aabb, bits, int G, long R, float dt, int k_max, count)
    with pytest.raises(TypeError):
        fn(None, None, None, None, None, 4, 0, 0.1, 8)  # one short
    with pytest.raises(ctypes.ArgumentError):
        fn(None, None, None, None, None, 4.0, 0, 0.1, 8, None)  # a float for `int G`


def test_load_is_cached():
    assert host_twin.load("occgrid") is host_twin.load("occgrid")
