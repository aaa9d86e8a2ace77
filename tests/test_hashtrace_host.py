"""Sphere tracing of the hash field's SDF on the CPU: the twin of the kernel (tests/host_harness/hashtrace/hashtrace_host.cpp, the same
csrc/hashtrace_math.hpp functions) against a float64 root search over oracle/hashgrid_oracle.py (tests/hashtrace_checks.py).  The bound on a hit
is |t_hit - t_ref| * len <= 5 eps: both ends satisfy |sdf| <= eps on a stretch where the directional derivative is at least 0.6 (the incidence
cosine of the ray sets) x ~0.9 (the interpolant's gradient norm).  The GPU suite (tests/test_gpu_zzzzzzzzzzhashtrace.py) holds the kernel to
this twin.  CPU only.

Measured, twin against float64, max |t_hit - t_ref| * len / eps over 128 hit rays: sphere 1.61, two spheres 1.96, sphere at F = 4 1.61; 4.6 to 4.8
evaluations per ray on average, 11 at most; every hit CONVERGED but one BRACKETED ray of the two spheres (the interpolant of a distance is
1-Lipschitz up to the min() crease and rounding: a step of the field's own size hardly ever overshoots)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashtrace_checks as TC  # noqa: E402
import host_twin  # noqa: E402

import lab4d_amd.hashtrace  # noqa: E402,F401  (the feature under test: its host layer must import without a GPU)

N_HIT, N_MISS = 128, 64


@pytest.fixture(scope="module")
def host():
    return TC.build_host()


def check_hits(name, t_hit, status, d):
    """shared with the GPU suite: status in {1, 2} on every ray of the HIT set, t_hit within the bound of the float64 root; returns the worst
    |t_hit - t_ref| * len / eps"""
    ref = TC.truth(name, "hit", N_HIT)
    left_out = ref["kind"] != "root"  # the criterion: the float64 field has no sign change from positive on the clipped ray
    assert left_out.mean() < 0.01 and not left_out.any(), ref["kind"][left_out]  # (the ray sets are chosen so that none is)
    assert np.isin(status, (TC.CONVERGED, TC.BRACKETED)).all(), np.unique(status, return_counts=True)
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    err = np.abs(t_hit.astype(np.float64) - ref["t_ref"]) * ln / TC.EPS
    print("%s: max |t_hit - t_ref| * len = %.3f eps, %d converged, %d bracketed" % (name, err.max(), (status == 1).sum(), (status == 2).sum()))
    assert err.max() <= TC.T_BOUND, err.max()
    return float(err.max())


@pytest.mark.parametrize("name", ["sphere", "two", "sphere4"])
def test_hit_rays_against_float64(host, name):
    P, cfg = TC.field(name)
    o, d, tr = TC.rays(name, "hit", N_HIT)
    b = TC.impact(o, d, TC.shape_of(name)[0])
    assert (b <= 0.8 * TC.shape_of(name)[1]).any(1).all()
    t_hit, status, n_eval, sdf_hit = TC.host_trace(host, P, cfg, o, d, tr)
    check_hits(name, t_hit, status, d)
    assert (n_eval >= 2).all() and (n_eval <= 128 + 8).all() and (np.abs(sdf_hit[status == 1]) <= TC.EPS).all()
    print("n_eval mean %.1f max %d" % (n_eval.mean(), n_eval.max()))


@pytest.mark.parametrize("name", ["sphere", "two", "sphere4"])
def test_miss_rays(host, name):
    P, cfg = TC.field(name)
    o, d, tr = TC.rays(name, "miss", N_MISS)
    assert (TC.impact(o, d, TC.shape_of(name)[0]) >= 1.3 * TC.shape_of(name)[1]).all()
    ref = TC.truth(name, "miss", N_MISS)
    assert (ref["kind"] == "none").all()  # the reference leaves out none
    t_hit, status, n_eval, sdf_hit = TC.host_trace(host, P, cfg, o, d, tr)
    t_clip, ok = TC.host_clip(host, o, d, tr, P)
    assert ok.all() and (status == TC.MISS).all() and np.array_equal(t_hit, t_clip[:, 1])
    assert np.abs(t_clip.astype(np.float64) - np.stack([ref["t_enter"], ref["t_exit"]], 1)).max() < 1e-5  # the fp32 slab against the float64 one
    assert (sdf_hit > TC.EPS).all() and (n_eval >= 2).all()


def test_statuses_3_and_4(host):
    P, cfg = TC.field("two")
    o, d, tr = TC.rays("two", "inside", 32)
    assert (TC.truth("two", "inside", 32)["kind"] == "inside").all()
    t_hit, status, n_eval, sdf_hit = TC.host_trace(host, P, cfg, o, d, tr)
    assert (status == TC.STARTS_INSIDE).all() and (n_eval == 1).all() and (sdf_hit <= 0).all() and np.array_equal(t_hit, TC.host_clip(host, o, d, tr, P)[0][:, 0])
    # one evaluation and no bisection: a ray that starts outside runs out of steps at t_enter
    o, d, tr = TC.rays("two", "hit", N_HIT)
    t_hit, status, n_eval, sdf_hit = TC.host_trace(host, P, cfg, o, d, tr, max_steps=1, n_bisect=0)
    assert (status == TC.OUT_OF_STEPS).all() and (n_eval == 1).all() and np.array_equal(t_hit, TC.host_clip(host, o, d, tr, P)[0][:, 0])
    # no bisection and a floor on the step that overshoots: BRACKETED at the raw step, behind the surface
    ref = TC.truth("two", "hit", N_HIT)
    t_hit, status, n_eval, sdf_hit = TC.host_trace(host, P, cfg, o, d, tr, min_step=0.004, n_bisect=0)
    assert np.isin(status, (TC.CONVERGED, TC.BRACKETED)).all()
    br = status == TC.BRACKETED
    assert br.sum() > N_HIT // 2 and (sdf_hit[br] < -TC.EPS).all() and (t_hit[br] > ref["t_ref"][br]).all()
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    assert ((t_hit[br] - ref["t_ref"][br]) * ln[br] <= 0.004 * (1 + 1e-5)).all()  # at most one floor step behind it
    # with the bisection the same rays come back to the surface: the bracket of 0.004 halved 8 times, over the directional derivative
    t8, s8, n8, _ = TC.host_trace(host, P, cfg, o, d, tr, min_step=0.004, n_bisect=8)
    assert np.isin(s8, (TC.CONVERGED, TC.BRACKETED)).all() and (n8 <= 128 + 8).all()
    assert (np.abs(t8 - ref["t_ref"]) * ln <= max(TC.T_BOUND * TC.EPS, 0.004 / 256)).all()


@pytest.mark.parametrize("name", ["sphere", "random"])
def test_invariants(host, name):
    P, cfg = TC.field(name)
    o, d, tr = TC.rays(name, "generic", 256)
    check_invariants(P, cfg, o, d, tr, TC.host_clip(host, o, d, tr, P), *TC.host_trace(host, P, cfg, o, d, tr), need_hits=name == "random")
    for kw in (dict(max_steps=5, n_bisect=3), dict(step_scale=0.5, min_step=0.002, n_bisect=32)):
        check_invariants(P, cfg, o, d, tr, TC.host_clip(host, o, d, tr, P), *TC.host_trace(host, P, cfg, o, d, tr, **kw), **kw)


def check_invariants(P, cfg, o, d, tr, clip, t_hit, status, n_eval, sdf_hit, max_steps=128, n_bisect=8, need_hits=False, **_):
    """shared with the GPU suite: t_enter <= t_hit <= t_exit, n_eval <= max_steps + n_bisect, |sdf64(p_hit)| <= eps + 1e-6 for status 1"""
    t_clip, ok = clip
    assert ok.all() and (t_clip[:, 0] <= t_hit).all() and (t_hit <= t_clip[:, 1]).all()
    assert (n_eval >= 1).all() and (n_eval <= max_steps + n_bisect).all() and np.isin(status, range(5)).all()
    s64 = TC.sdf64(P, cfg, torch.from_numpy(TC.point_at(o, d, t_hit)).double()).numpy()
    conv = status == TC.CONVERGED
    print("statuses", np.bincount(status, minlength=5), "max |sdf64| at CONVERGED %.3e" % (np.abs(s64[conv]).max() if conv.any() else 0.0))
    assert (np.abs(s64[conv]) <= TC.EPS + 1e-6).all()
    assert np.abs(s64 - sdf_hit).max() <= 1e-6  # sdf_hit is the field at t_hit
    assert (s64[status == TC.STARTS_INSIDE] <= 1e-6).all() and (s64[status == TC.MISS] > 0).all()
    if need_hits:
        assert conv.sum() + (status == TC.BRACKETED).sum() > 32


def test_degenerate_rays(host):
    P, cfg = TC.field("sphere")
    o, d, tr, _ = TC.degenerate_rays()
    TC.check_degenerate(*TC.host_trace(host, P, cfg, o, d, tr))
    TC.check_degenerate(*TC.host_trace(host, P, cfg, o, d, tr, max_steps=1024, n_bisect=0), max_steps=1024, n_bisect=0)
    out = TC.host_trace(host, P, cfg, o[:0], d[:0], tr[:0])  # R = 0
    assert all(a.size == 0 for a in out)
    for kw in (dict(eps=0.0), dict(eps=float("nan")), dict(step_scale=0.0), dict(step_scale=1.5), dict(min_step=0.0), dict(max_steps=0), dict(max_steps=1025),
               dict(n_bisect=-1), dict(n_bisect=33)):
        TC.host_trace(host, P, cfg, o, d, tr, expect=-1, **kw)


def test_twin_runs_clean_under_the_sanitizers():
    """the stand-alone program over the degenerate rays of the rules, AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU"""
    r = subprocess.run([host_twin.sanitized_main("hashtrace")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hashtrace_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_trace_kernel_uses_no_scratch(tmp_path):
    """csrc/hashtrace.hip compiled for gfx950 as the build does: k_hashsdf_trace once per F in 1, 2, 4, 8, no private segment and no spills,
    at least three waves per SIMD; the figures go to profiles/hashtrace_kernel_resources.txt"""
    kernels = host_twin.kernel_metadata("hashtrace.hip", tmp_path)
    assert len(kernels) == 4 and all("k_hashsdf_trace" in k["name"] for k in kernels), kernels
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "agpr_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
    assert max(k["vgpr_count"] for k in kernels) <= 168, kernels  # 512 / 3 rounded down to the granule of 8
    asm, = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "amdgcn" in f]
    text = open(tmp_path / asm).read()
    lds = [int(x) for x in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", text)]
    occ = [int(x) for x in re.findall(r"^; Occupancy: (\d+)", text, flags=re.M)]
    assert len(lds) == len(occ) == 4 and set(lds) == {(64 * 32 + 64 + 64) * 4} and min(occ) >= 3, (lds, occ)
    lines = ["k_hashsdf_trace<%d>  V %d A %d scratch %d spill %d LDS %d occ %d\n" % (f, k["vgpr_count"], k["agpr_count"], k["private_segment_fixed_size"],
                                                                                   k["vgpr_spill_count"] + k["sgpr_spill_count"], b, w)
             for f, k, b, w in zip((1, 2, 4, 8), kernels, lds, occ)]
    path = os.path.join(host_twin._lib.ROOT, "profiles", "hashtrace_kernel_resources.txt")
    if not os.path.exists(path) or open(path).read() != "".join(lines):
        with open(path, "w") as fh:
            fh.writelines(lines)


def test_host_layer_checks_its_arguments():
    from lab4d_amd import hashfield, hashtrace
    P, cfg = TC.field("sphere")
    o, d, tr = (torch.from_numpy(a) for a in TC.rays("sphere", "hit", N_HIT))
    res = torch.tensor(TC.res_list(cfg), dtype=torch.int32)
    net = (P["hash.geo.0.weight"], P["hash.geo.0.bias"], P["hash.geo.2.weight"][0], P["hash.geo.2.bias"][:1])
    args = (o, d, tr, P["aabb"], P["hash.table"], res, cfg["log2_T"]) + net
    with pytest.raises(RuntimeError, match="no CPU path"):
        hashtrace.trace(*args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hashfield.trace_surface(P, cfg, o, d, tr)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hashfield.render_surface(P, cfg, o, d, tr)
    with pytest.raises(NotImplementedError, match="L\\*F = 32"):
        hashfield.trace_surface(P, dict(cfg, L=8), o, d, tr)
    with pytest.raises(RuntimeError, match=r"origin must be float32 \(R, 3\)"):
        hashtrace.trace(o.double(), *args[1:])
    with pytest.raises(RuntimeError, match="disagree"):
        hashtrace.trace(o, d, tr[:5], *args[3:])
    with pytest.raises(RuntimeError, match=r"aabb must be float32 \(2, 3\)"):
        hashtrace.trace(o, d, tr, P["aabb"].reshape(-1), *args[4:])
    with pytest.raises(RuntimeError, match=r"L \* F = 32"):
        hashtrace.trace(o, d, tr, P["aabb"], P["hash.table"][:8], res[:8], cfg["log2_T"], *net)
    with pytest.raises(RuntimeError, match="2\\^log2_T rows"):
        hashtrace.trace(o, d, tr, P["aabb"], P["hash.table"], res, cfg["log2_T"] + 1, *net)
    with pytest.raises(RuntimeError, match=r"w2 must be float32 \(64,\)"):
        hashtrace.trace(*args[:9], P["hash.geo.2.weight"], net[3])
    for kw, msg in ((dict(eps=0.0), "eps = 0.0 must be finite"), (dict(eps=float("inf")), "eps = inf"), (dict(step_scale=1.5), r"step_scale = 1.5 outside \(0, 1\]"),
                    (dict(min_step=-1.0), "min_step = -1.0"), (dict(max_steps=0), r"max_steps = 0 outside \[1, 1024\]"),
                    (dict(max_steps=1025), "max_steps = 1025"), (dict(n_bisect=33), r"n_bisect = 33 outside \[0, 32\]")):
        with pytest.raises(RuntimeError, match=msg):
            hashtrace.trace(*args, **kw)
    assert (hashtrace.MISS, hashtrace.CONVERGED, hashtrace.BRACKETED, hashtrace.STARTS_INSIDE, hashtrace.OUT_OF_STEPS) == tuple(range(5))


def test_c_abi_checks_its_arguments_before_any_launch():
    """the entry point refuses bad arguments with the library's error code and a message; nothing is launched (no GPU here); R = 0 succeeds"""
    from lab4d_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(origin=p, dir=p, t_range=p, aabb=p, R=4, table=p, res=p, L=16, log2_T=12, F=2, W1=p, b1=p, w2=p, b2=p, eps=1e-4, step_scale=1.0, min_step=1e-4,
              max_steps=128, n_bisect=8, t_hit=p, status=p, n_eval=p, sdf_hit=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.lab4d_hashsdf_trace(*[a[k] for k in ok], None)

    cases = [(dict(R=-1), "R = -1"), (dict(L=8), "L = 8, F = 2"), (dict(L=2, F=16), "F = 16"), (dict(log2_T=3), "log2_T = 3"), (dict(log2_T=25), "log2_T = 25"),
             (dict(eps=0.0), "eps = 0"), (dict(eps=float("nan")), "eps = nan"), (dict(step_scale=0.0), "step_scale = 0"), (dict(step_scale=1.25), "step_scale = 1.25"),
             (dict(min_step=0.0), "min_step = 0"), (dict(min_step=float("inf")), "min_step = inf"), (dict(max_steps=0), "max_steps = 0"),
             (dict(max_steps=1025), "max_steps = 1025"), (dict(n_bisect=-1), "n_bisect = -1"), (dict(n_bisect=33), "n_bisect = 33"),
             (dict(origin=None), "null pointer (origin"), (dict(aabb=None), "null pointer (aabb"), (dict(table=None), "null pointer (aabb"),
             (dict(b2=None), "null pointer (W1"), (dict(t_hit=None), "null pointer (t_hit"), (dict(sdf_hit=None), "null pointer (t_hit")]
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in lib.lab4d_last_error().decode(), (msg, lib.lab4d_last_error().decode())
    assert call(R=0) == 0 and call(R=0, origin=None, dir=None, t_range=None, t_hit=None, status=None, n_eval=None, sdf_hit=None) == 0
    assert call(R=0, W1=None) == -1
    assert _lib.SIGNATURES["lab4d_hashsdf_trace"][1][4] is ctypes.c_long and _lib.SIGNATURES["lab4d_hashsdf_trace"][2]
