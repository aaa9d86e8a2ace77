"""CPU twin of the distortion loss (tests/host_harness/distort/distort_host.cpp over lab4d_amd/csrc/distort_math.hpp) against the definition of
include/lab4d_distort.h in torch float64 (tests/distort_checks.py: the O(n^2) double sum per ray with autograd), within the project's fp32
bar.  The GPU suite holds the kernels to the same reference and to this twin (tests/test_gpu_zzzzzzzzzdistort.py).  No GPU.

Measured (rel_max of the twin against float64; loss / g_density / g_deltas): composite_case 4.1e-7 / 1.8e-6 / 2.1e-6; the ragged list at
R = 1, 63, 64, 65, 400: at most 7.6e-7 / 3.6e-6 / 6.3e-6."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distort_checks as DC  # noqa: E402
import host_twin  # noqa: E402
import packed_checks as PC  # noqa: E402


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_twin_against_float64_on_the_composite_list():
    case = DC.composite_list(seed=4)
    DC.check(DC.host_distortion(DC.build_host(), case), DC.ref_distortion(case), "twin, composite_case")


@pytest.mark.parametrize("R", [1, 63, 64, 65, 400])
def test_twin_against_float64_on_the_ragged_list(R):
    case = DC.ragged_list(R, seed=100 + R)
    ref = DC.ref_distortion(case)
    DC.check(DC.host_distortion(DC.build_host(), case), ref, "twin, ragged R = %d" % R)
    assert R < 63 or (ref["loss"] > 0).sum() > R // 2


def test_invariants():
    lib = DC.build_host()
    case = DC.ragged_list(100, seed=5)
    got = DC.host_distortion(lib, case)
    n = np.array([DC.rows_of(case, r)[1] for r in range(case["R"])])
    assert (n == 0).sum() >= 2 and (got["loss"][n == 0] == 0).all()  # a ray of 0 rows (the one in front of the list among them)
    assert (got["loss"] >= 0).all() and (got["loss"][n > 0] > 0).all() and np.isfinite(got["loss"]).all()
    # a ray of 1 row: (1/3) w^2 width in the order distort_math.hpp states it, on the compositor twin's own weight of that row
    w = PC.host_composite(PC.build_host(), case["density"], case["deltas"], [], [], case["start"], case["count"])["weights"]
    singles = np.flatnonzero(n == 1)
    assert len(singles) >= 3
    for r in singles:
        s = DC.rows_of(case, r)[0]
        assert got["loss"][r] == np.float32(1.0 / 3.0) * w[s] * w[s] * case["width"][s] and w[s].dtype == np.float32, r
    # each gradient alone equals the pair's
    for k in ("g_density", "g_deltas"):
        alone = DC.host_distortion(lib, case, which=(k,))
        assert sorted(alone) == sorted(("loss", k)) and np.array_equal(words(alone[k]), words(got[k])), k


def test_a_constant_added_to_mid_changes_no_bit():
    """the shift by the ray's first midpoint: on midpoints that are multiples of 2^-12 below 16, adding 16 is exact in fp32, so the shifted
    midpoints -- all the kernel and the twin ever see of mid -- are the same words, and with them loss and gradients"""
    lib = DC.build_host()
    case = DC.ragged_list(65, seed=9)
    case["mid"] = (np.round(case["mid"].astype(np.float64) * 4096) / 4096).astype(np.float32)
    assert float(case["mid"].max()) < 16 and np.array_equal(case["mid"].astype(np.float64) * 4096 % 1, np.zeros(case["P"]))
    moved = dict(case, mid=case["mid"] + np.float32(16))
    assert np.array_equal(moved["mid"].astype(np.float64), case["mid"].astype(np.float64) + 16)
    a, b = DC.host_distortion(lib, case), DC.host_distortion(lib, moved)
    for k in DC.OUTPUTS:
        assert np.array_equal(words(a[k]), words(b[k])), k
    assert a["loss"].max() > 0 and np.abs(a["g_density"]).max() > 0


def test_rows_of_no_ray_are_neither_read_nor_written():
    """NaN in every input row that no ray owns, a sentinel in the gradient rows: the results are those of the clean list, the sentinel stays"""
    lib = DC.build_host()
    case = DC.ragged_list(65, seed=12)
    dirty = DC.poisoned(case)
    assert 5 < (~dirty["owned"]).sum() < case["P"] // 2
    clean, got = DC.host_distortion(lib, case, sentinel=-7.0), DC.host_distortion(lib, dirty, sentinel=-7.0)
    for k in DC.OUTPUTS:
        assert np.array_equal(words(clean[k]), words(got[k])), k
    for k in DC.OUTPUTS[1:]:
        assert (got[k][~dirty["owned"]] == -7.0).all() and (got[k][dirty["owned"]] != -7.0).all(), k
    DC.check({k: np.where(dirty["owned"], got[k], 0) if k != "loss" else got[k] for k in DC.OUTPUTS}, DC.ref_distortion(dirty), "twin, poisoned")


def test_no_rays_and_no_rows():
    lib = DC.build_host()
    case = DC.ragged_list(5, seed=1)
    none = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    none.update(R=0, P=0)
    got = DC.host_distortion(lib, none)
    assert got["loss"].shape == (0,) and got["g_density"].shape == (0,)
    empty = {k: (v[:0] if isinstance(v, np.ndarray) and k not in ("start", "count", "g_loss") else v) for k, v in case.items()}
    empty["P"] = 0
    got = DC.host_distortion(lib, empty)
    assert (got["loss"] == 0).all() and got["loss"].shape == (5,)
    assert (DC.ref_distortion(empty)["loss"] == 0).all()


def test_call_sites_and_prototypes_of_the_two_entry_points():
    """the ABI walk of tests/test_abi.py for the new launch sites: both entry points are declared with a stream, their signatures are the
    pinned ones, and lab4d_amd/packed.py calls each once with as many arguments as the prototype has in front of its stream; the twin's
    definitions take the same parameters, stream aside, and every extern "C" function of the twin is typed from its source"""
    import ast
    import ctypes
    from lab4d_amd import _lib
    vp, cl, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    pinned = {"lab4d_packed_distortion_forward": (ci, [vp] * 6 + [cl, cl, vp, vp], True),
              "lab4d_packed_distortion_backward": (ci, [vp] * 6 + [cl, cl, vp, vp, vp, vp], True)}
    for name, want in pinned.items():
        restype, params, has_stream = _lib.SIGNATURES[name]
        assert (restype, _lib.argtypes(params), has_stream) == want, name
    sites = {}
    for node in ast.walk(ast.parse(open(os.path.join(_lib.HERE, "packed.py")).read())):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call" and isinstance(node.func.value, ast.Name)
                and node.func.value.id == "_lib" and isinstance(node.args[0], ast.Constant) and node.args[0].value.startswith("packed_distortion_")):
            assert not any(isinstance(a, ast.Starred) for a in node.args)
            sites.setdefault(node.args[0].value, []).append(len(node.args) - 1)
    assert sites == {"packed_distortion_forward": [9], "packed_distortion_backward": [11]}, sites
    with open(os.path.join(host_twin.HARNESS, DC.TWIN + "_host.cpp")) as fh:
        text = fh.read()
    twin = host_twin.signatures(text, DC.TWIN + "_host.cpp")
    assert sorted(twin) == ["distort_host_backward", "distort_host_forward"] and text.count('extern "C"') == 2  # (every function of the twin is typed)
    lib = DC.build_host()
    for name in ("forward", "backward"):
        assert twin["distort_host_" + name][1] == _lib.argtypes(_lib.SIGNATURES["lab4d_packed_distortion_" + name][1])[:-1], name
        assert list(getattr(lib, "distort_host_" + name).argtypes) == twin["distort_host_" + name][1] and getattr(lib, "distort_host_" + name).restype is None


def test_twin_runs_clean_under_the_sanitizers():
    """the stand-alone program over the empty rays, the chunk edges, the (start, count) that leave [0, P), each gradient alone, R = 0 and
    P = 0; AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU"""
    r = subprocess.run([host_twin.sanitized_main("distort")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "distort_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_kernels_have_no_private_segment_and_no_spills(tmp_path):
    kernels = host_twin.kernel_metadata("distort.hip", tmp_path)
    names = [k["name"] for k in kernels]
    assert len(names) == 2 and all(any(n in x for x in names) for n in ("k_packed_distortion_fwd", "k_packed_distortion_bwd")), names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "agpr_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
    assert max(k["vgpr_count"] for k in kernels) <= 64, kernels  # eight waves per SIMD
