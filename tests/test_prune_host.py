"""CPU twin of the prune (tests/host_harness/prune/prune_host.cpp over lab4d_amd/csrc/prune_math.hpp) against the rules of include/lab4d_prune.h
restated in float64 (tests/prune_checks.py).  The GPU suite holds the kernels to this twin (tests/test_gpu_zzzzzzzzprune.py); here the twin
itself is pinned.  No GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import prune_checks as PR  # noqa: E402


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("eps", PR.EPS)
@pytest.mark.parametrize("alpha", PR.ALPHA)
def test_twin_keeps_the_float64_set_on_generic_rays(eps, alpha):
    """deltas 1/64, densities uniform in [0, 200], three rays in ten thinner by 20 or 50: 77 % (eps 1e-4) and 90 % (eps 1e-2) of the rays of
    63 rows or more reach the stop, 14 to 41 rays keep rows behind their first chunk.  The excluded share is a condition (< 1 %); measured:
    0 of 400 rays at every pair with this seed."""
    lib = PR.build_host()
    case = PR.make_list(400, seed=11)
    tau_stop, tau_min = PR.thresholds(eps, alpha)
    got = PR.host_prune(lib, case, tau_stop, tau_min)
    keep, generic, stop_at = PR.ref_keep(case, tau_stop, tau_min)
    excluded = 1.0 - generic.mean()
    stopped = long_rays = late = 0
    for r in range(case["R"]):
        s, n = PR.rows_of(case, r)
        if n >= 63:
            long_rays += 1
            stopped += stop_at[r] >= 0
            late += bool(keep[s + 64:s + n].any())  # survivors behind the first chunk: the carry decides their stop
        if generic[r]:
            assert np.array_equal(got["keep"][s:s + n].astype(bool), keep[s:s + n]), r
            assert got["count"][r] == keep[s:s + n].sum()
    print("eps %g alpha %g: %d rays, excluded share %.4f, %d of %d rays of >= 63 rows reach the stop, %d keep rows behind their first chunk, %d of %d rows kept"
          % (eps, alpha, case["R"], excluded, stopped, long_rays, late, got["total"], case["P"]))
    assert excluded < 0.01, excluded
    assert stopped > 0.6 * long_rays and late >= 10 and 0 < got["total"] < case["P"] // 2


@pytest.mark.parametrize("eps,alpha", [(1e-4, 0.0), (1e-2, 0.05), (0.0, 1e-3)])
def test_twin_invariants(eps, alpha):
    lib = PR.build_host()
    case = PR.make_list(100, seed=5)
    tau_stop, tau_min = PR.thresholds(eps, alpha)
    got = PR.host_prune(lib, case, tau_stop, tau_min)
    n = got["total"]
    assert n == got["count"].sum() == got["keep"].sum() and not got["overflow"] and np.array_equal(got["ray_count"], got["count"])
    assert np.array_equal(got["ray_start"], np.cumsum(got["count"]) - got["count"])
    src = got["src_row"]
    assert np.array_equal(np.flatnonzero(got["keep"]), np.sort(src))  # the survivors are the kept rows ...
    for k in ("t", "deltas", "xyz", "dirs"):  # ... and copy their source row bit for bit
        assert np.array_equal(words(got[k]), words(case[k][src])), k
    assert np.array_equal(got["ray_idx"], np.repeat(np.arange(case["R"], dtype=np.int32), got["count"]))
    same_ray = got["ray_idx"][1:] == got["ray_idx"][:-1]
    assert (np.diff(src)[same_ray] > 0).all() and same_ray.sum() > 50  # strictly ascending inside a ray
    tau = case["density"].astype(np.float64) * case["deltas"]
    for r in range(case["R"]):
        s, m = PR.rows_of(case, r)
        mine = src[got["ray_start"][r]:got["ray_start"][r] + got["count"][r]]
        assert ((mine >= s) & (mine < s + m)).all()
        if tau_min == 0:  # a prefix of the ray's rows ...
            assert np.array_equal(mine, np.arange(s, s + got["count"][r]))
            if got["count"][r] < m:  # ... that ends in front of the stop row: its exclusive prefix lies above tau_stop, the last survivor's does not
                k = got["count"][r]
                assert tau[s:s + k].sum() > tau_stop * (1 - 1e-6) and (k == 0 or tau[s:s + k - 1].sum() <= tau_stop * (1 + 1e-6))
    assert (got["count"][case["count"] == 0] == 0).all() and got["count"][-1] == 0 and got["count"][-2] <= 5  # empty rays, the two that leave [0, P)
    # the capacities: total, total - 1, 0 (and room to spare)
    last = int(np.nonzero(got["count"])[0][-1])
    for cap in (n, n - 1, 0, n + 5):
        cut = PR.host_prune(lib, case, tau_stop, tau_min, cap=cap)
        assert cut["total"] == n and cut["overflow"] == (n > cap)
        m = min(cap, n)
        want = got["count"].copy()
        if cap == n - 1:
            want[last] -= 1
        elif cap == 0:
            want[:] = 0
        assert np.array_equal(cut["ray_count"], want) and cut["ray_count"].sum() == m
        for k in ("t", "deltas", "xyz", "dirs", "ray_idx", "src_row"):
            assert np.array_equal(words(cut[k][:m]), words(got[k][:m])), (cap, k)
        # parked rows, as the march parks them
        assert (cut["ray_idx"][m:] == -1).all() and (cut["src_row"][m:] == -1).all() and (cut["t"][m:] == 0).all() and (cut["deltas"][m:] == 0).all()
        lo, hi = PR.AABB[:3], PR.AABB[3:]
        assert np.array_equal(cut["xyz"][m:], np.broadcast_to((hi + (hi - lo)).astype(np.float32), (cap - m, 3)))
        assert np.array_equal(cut["dirs"][m:], np.broadcast_to(np.float32([0, 0, 1]), (cap - m, 3)))


def test_both_rules_off_is_the_identity():
    """eps = 0, alpha = 0 on finite positive densities and a list without gaps: every array word for word, ray_start included"""
    lib = PR.build_host()
    case = PR.make_list(60, seed=2, gaps=False, out_of_range=False)
    case["density"] = np.maximum(case["density"], np.float32(1e-3))
    tau_stop, tau_min = PR.thresholds(0.0, 0.0)
    assert tau_stop == math.inf and tau_min == 0.0
    got = PR.host_prune(lib, case, tau_stop, tau_min)
    assert got["total"] == case["P"] and got["keep"].all()
    assert np.array_equal(got["ray_start"], case["start"]) and np.array_equal(got["ray_count"], case["count"])
    assert np.array_equal(got["src_row"], np.arange(case["P"], dtype=np.int32))
    for k in ("t", "deltas", "xyz", "dirs"):
        assert np.array_equal(words(got[k]), words(case[k])), k


def test_nan_and_negative_density_count_as_tau_zero():
    lib = PR.build_host()
    case = PR.make_list(40, seed=3)
    rng = np.random.default_rng(0)
    bad = rng.random(case["P"]) < 0.3
    clean = dict(case, density=np.where(bad, np.float32(0), case["density"]))
    dirty = dict(case, density=np.where(bad, rng.choice(np.float32([np.nan, -1.0, -np.inf, -0.0]), case["P"]), case["density"]).astype(np.float32))
    for eps, alpha in ((1e-4, 0.0), (1e-2, 1e-3)):
        a, b = PR.host_prune(lib, clean, *PR.thresholds(eps, alpha)), PR.host_prune(lib, dirty, *PR.thresholds(eps, alpha))
        assert np.array_equal(a["keep"], b["keep"]) and np.array_equal(a["src_row"], b["src_row"]) and a["total"] == b["total"] > 0
        assert (a["keep"][bad] == 0).all() if alpha > 0 else a["keep"][bad].any()  # tau = 0: below any tau_min > 0, kept in front of the stop otherwise


def test_no_rays_and_no_rows():
    lib = PR.build_host()
    case = PR.make_list(0, seed=1, out_of_range=False)
    got = PR.host_prune(lib, case, 1.0, 0.0, cap=3)
    assert got["total"] == 0 and not got["overflow"] and (got["ray_idx"] == -1).all() and (got["src_row"] == -1).all()
    case = PR.make_list(5, seed=1, out_of_range=False)
    empty = {k: (v[:0] if isinstance(v, np.ndarray) and k not in ("start", "count") else v) for k, v in case.items()}
    empty["P"] = 0
    got = PR.host_prune(lib, empty, 1.0, 0.0, cap=3)
    assert got["total"] == 0 and (got["ray_count"] == 0).all() and (got["ray_idx"] == -1).all()


def test_thresholds_are_formed_in_double_and_refused_outside_the_unit_interval():
    from lab4d_amd import packed
    for eps in PR.EPS + (0.0,):
        for alpha in PR.ALPHA:
            assert packed.prune_thresholds(eps, alpha) == PR.thresholds(eps, alpha)
    assert packed.prune_thresholds(1e-4, 0.05) == (float(np.float32(-math.log(1e-4))), float(np.float32(-math.log1p(-0.05))))
    for eps, alpha in ((1.0, 0.0), (-0.1, 0.0), (float("nan"), 0.0), (1e-4, 1.0), (1e-4, -1e-3), (1e-4, float("nan"))):
        with pytest.raises(RuntimeError, match="outside"):
            packed.prune_thresholds(eps, alpha)


def test_call_sites_and_prototypes_of_the_two_entry_points():
    """the ABI walk of tests/test_abi.py for the new launch sites: both entry points are declared with a stream (tests/test_abi.py pins the
    set without one), their signatures are the pinned ones, and lab4d_amd/packed.py calls each once with as many arguments as the prototype
    has in front of its stream; the twin's definitions take the same parameters, stream aside"""
    import ast
    import ctypes
    from lab4d_amd import _lib
    vp, cl, cf, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_int
    pinned = {"lab4d_packed_prune_count": (ci, [vp, vp, vp, vp, cl, cl, cf, cf, vp, vp, vp], True),
              "lab4d_packed_prune_write": (ci, [vp] * 4 + [cl] * 3 + [vp] * 15, True)}
    for name, want in pinned.items():
        restype, params, has_stream = _lib.SIGNATURES[name]
        assert (restype, _lib.argtypes(params), has_stream) == want, name
    sites = {}
    for node in ast.walk(ast.parse(open(os.path.join(_lib.HERE, "packed.py")).read())):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call" and isinstance(node.func.value, ast.Name)
                and node.func.value.id == "_lib" and isinstance(node.args[0], ast.Constant) and node.args[0].value.startswith("packed_prune_")):
            assert not any(isinstance(a, ast.Starred) for a in node.args)
            sites.setdefault(node.args[0].value, []).append(len(node.args) - 1)
    assert sites == {"packed_prune_count": [10], "packed_prune_write": [21]}, sites
    with open(os.path.join(host_twin.HARNESS, PR.TWIN + "_host.cpp")) as fh:
        text = fh.read()
    twin = host_twin.signatures(text, PR.TWIN + "_host.cpp")
    assert sorted(twin) == ["prune_host_count", "prune_host_write"] and text.count('extern "C"') == 2  # (every function of the twin is typed)
    lib = PR.build_host()
    for name in ("count", "write"):
        assert twin["prune_host_" + name][1] == _lib.argtypes(_lib.SIGNATURES["lab4d_packed_prune_" + name][1])[:-1], name
        assert list(getattr(lib, "prune_host_" + name).argtypes) == twin["prune_host_" + name][1] and getattr(lib, "prune_host_" + name).restype is None


def test_twin_runs_clean_under_the_sanitizers():
    """the stand-alone program over the truncation cases, the empty rays, the (start, count) that leave [0, P), R = 0 and P = 0;
    AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU"""
    r = subprocess.run([host_twin.sanitized_main("prune")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "prune_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_kernels_have_no_private_segment_and_no_spills(tmp_path):
    kernels = host_twin.kernel_metadata("prune.hip", tmp_path)
    names = [k["name"] for k in kernels]
    assert len(names) == 3 and all(any(n in x for x in names) for n in ("k_packed_prune_count", "k_packed_prune_write", "k_packed_prune_park")), names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "agpr_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
    assert max(k["vgpr_count"] for k in kernels) <= 64, kernels  # "a few dozen": eight waves per SIMD
