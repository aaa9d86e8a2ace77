"""The footprint-weighted hash encoding on the CPU: level_weight's properties, the twin of the AA kernels (tests/host_harness/hashaa/hashaa_host.cpp, the
same csrc/hashgrid_math.hpp functions) against the float64 definition in numpy (tests/hashaa_checks.py), the twin at radius 0 against the
unweighted twin bit for bit, the stand-alone program under the sanitizers, the host layer's argument checks and the C ABI's.  The GPU suite
(tests/test_gpu_zzzzzzzzzzzzzzzzzzhashaa.py) holds the kernels to the same float64 truth, with this twin's error as the yardstick.  CPU only."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashaa_checks as AC  # noqa: E402
import host_twin  # noqa: E402

from lab4d_amd import hashfield, hashgrid  # noqa: E402  (the feature under test: its host layer must import without a GPU)


@pytest.fixture(scope="module")
def host():
    return AC.build_host()


def weight(host, radius, res, w_min=0.0):
    return host.hashaa_host_level_weight(radius, res, w_min)


def test_level_weight_properties(host):
    for res in (1, 16, 2048):
        for w_min in (0.0, 1.0 / 256, 1.0):
            assert weight(host, 0.0, res, w_min) == 1.0 and weight(host, -1.0, res, w_min) == 1.0 and weight(host, float("nan"), res, w_min) == 1.0
            assert weight(host, float("inf"), res, w_min) == 0.0
    # monotone non-increasing in the radius and in the resolution; within float32 rounding of the float64 definition
    radii = np.exp(np.linspace(math.log(1e-6), math.log(100.0), 400)).astype(np.float32)
    resolutions = [1, 4, 16, 17, 64, 511, 512, 2048]
    w = np.array([[weight(host, float(r), n) for n in resolutions] for r in radii])
    assert (np.diff(w, axis=0) <= 0).all() and (np.diff(w, axis=1) <= 0).all()
    assert w.max() == 1.0 and 0 < w.min() < 1e-5
    ref = AC.ref_weights(radii, resolutions, 0.0)
    assert np.abs(w - ref).max() < 4e-7  # (erff within a few ulp of 1, the quotient's three roundings)
    # the cut is per sample: exactly the entries below w_min go to zero, the others keep their value
    for w_min in (1.0 / 256, 0.5):
        cut = np.array([[weight(host, float(r), n, w_min) for n in resolutions] for r in radii])
        below = w < np.float32(w_min)
        assert below.any() and (~below).any()
        assert (cut[below] == 0).all() and (cut[~below] == w[~below]).all()
    assert weight(host, 0.01, 16, 1.0) == 0.0 and weight(host, 1e-30, 16, 1.0) == 1.0  # (w_min = 1 keeps only w = 1)


def test_torch_level_weights_follow_the_rule(host):
    rad = torch.from_numpy(np.concatenate([AC.radius("loguniform", 300), [0.0, -2.0]]).astype(np.float32))
    res = AC.res_list("a")
    for w_min in AC.W_MINS:
        w = hashgrid.level_weights(rad, res, w_min)
        assert tuple(w.shape) == (302, 16) and w.dtype == torch.float32
        ref = AC.ref_weights(rad.numpy(), res, w_min)
        twin = np.array([[weight(host, float(r), n, w_min) for n in res] for r in rad.numpy()])
        near_cut = np.abs(ref - w_min) < 1e-6  # (an entry within rounding of the cut may fall on either side)
        assert np.abs(w.numpy() - ref)[~near_cut].max() < 4e-7 and np.abs(twin - ref)[~near_cut].max() < 4e-7
        assert bool((w[[6, 7, 300, 301]] == 1).all()) and bool((w[8] == 0).all())
        assert torch.equal(hashgrid.level_weights(rad.reshape(2, 151), torch.tensor(res, dtype=torch.int32), w_min), w.reshape(2, 151, 16))
        assert torch.equal(AC.torch_weights(rad, res, w_min), w)


@pytest.mark.parametrize("inside_only", [False, True])
@pytest.mark.parametrize("w_min", AC.W_MINS)
@pytest.mark.parametrize("pattern", AC.PATTERNS)
@pytest.mark.parametrize("name", sorted(AC.CONFIGS))
def test_twin_against_float64(name, pattern, w_min, inside_only):
    """out and g_x to a few float32 roundings of their scale, the table gradient to 1e-6 relative L2 per level (serial fp32 sums of at most a
    few hundred terms); exact zeros where the definition has zeros"""
    c = AC.case(name, pattern, w_min, inside_only)
    L, F, log2_T, _, _ = c["cfg"]
    scale_out, scale_gx = np.abs(c["ref_out"]).max(), np.abs(c["ref_gx"]).max()
    print(name, pattern, w_min, inside_only, "twin errors: out %.2e (scale %.2e), g_x %.2e (scale %.2e)" % (c["yard_out"], scale_out, c["yard_gx"], scale_gx))
    # out: a blend of 8 products of 3 weights each, one more product with a weight that carries the quotient's and erff's roundings -- some 16
    # roundings of 2^-24 on terms no larger than the scale: 1e-6 of it.  g_x: L * 8 * (F + 4) such terms times res, summed with cancellation: 1e-5.
    assert c["yard_out"] <= 1e-6 * max(scale_out, 1e-30) and c["yard_gx"] <= 1e-5 * max(scale_gx, 1e-30)
    assert ((c["twin_out"] == 0) == (c["ref_out"] == 0)).all()
    ref, twin, err = AC.table_gradients(c, AC.N_ROWS)
    assert err.max() < 1e-6, err
    if pattern == "inf":
        assert not c["twin_out"].any() and not twin.any() and not c["twin_gx"].any()
    else:
        assert scale_out > 0.05 and scale_gx > 1.0
    if inside_only:
        outside = ~AC.inside01(c["x"])
        assert outside.sum() == 4 and not c["twin_out"][outside].any()
    if pattern == "raylike" and w_min > 0:  # whole runs of 64 rows are cut at the finest level and alive at the coarsest
        w = AC.ref_weights(c["radius"], c["res"], w_min).reshape(-1)[: 15 * 64 * L].reshape(15, 64, L)
        assert (w[:, :, -1] == 0).all(1).any() and (w[0, :, -1] == 0).all() and (w[0, :, 0] > 0).all()


@pytest.mark.parametrize("name", sorted(AC.CONFIGS))
def test_twin_at_radius_zero_equals_the_unweighted_twin_bit_for_bit(name):
    plain = host_twin.load("hashgrid")
    c = AC.case(name, "zero", 0.0, False)
    L, F, log2_T, _, _ = c["cfg"]
    x, tab, res, g = c["x"], c["table"], np.asarray(c["res"], np.int32), c["g_out"]
    S = x.shape[0]
    out = np.empty((S, L * F), np.float32)
    plain.hashgrid_host_forward(x.ctypes.data, tab.ctypes.data, res.ctypes.data, S, L, log2_T, F, out.ctypes.data)
    g_table, g_x = np.zeros_like(tab), np.empty_like(x)
    plain.hashgrid_host_backward(x.ctypes.data, tab.ctypes.data, res.ctypes.data, g.ctypes.data, S, L, log2_T, F, g_table.ctypes.data, g_x.ctypes.data)
    words = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for w_min in (0.0, 1.0 / 256, 1.0):  # (a point sample's weight is 1 whatever the cut)
        lib = AC.build_host()
        assert np.array_equal(words(AC.host_forward(lib, x, c["radius"], tab, res, log2_T, w_min, False)), words(out))
        gt, gx = AC.host_backward(lib, x, c["radius"], tab, res, log2_T, w_min, g)
        assert np.array_equal(words(gt), words(g_table)) and np.array_equal(words(gx), words(g_x))


def test_twin_runs_clean_under_the_sanitizers():
    """the stand-alone program (sizes 0, 1, 65; radius 0, inf, NaN, mixed), AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU"""
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(AC.TWIN)), exist_ok=True)
    r = subprocess.run([host_twin.sanitized_main(AC.TWIN)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hashaa_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_no_weighted_kernel_spills(tmp_path):
    """csrc/hashgrid.hip compiled for gfx950 as the build does: the five AA instantiations exist beside the five they were templated from; none
    of the ten spills a vector register; an AA instantiation parks no more scalar registers in VGPR lanes than its unweighted sibling (the
    unweighted k_hashgrid_bwd parks 6 kernel arguments in its prologue, as it did before the flag; every other kernel none) and has its
    sibling's private segment (the 16 bytes of the two backward kernels are the gx[3] array behind a selected pointer, not a spill)."""
    kernels = host_twin.kernel_metadata("hashgrid.hip", tmp_path)
    names = [k["name"] for k in kernels]
    for kernel, n in (("k_hashgrid_fwdILb", 4), ("k_hashgrid_fwd_lmILb", 2), ("k_hashgrid_bwdILb", 2), ("k_hashgrid_bwd_h2ILb", 2)):
        assert sum(kernel in x for x in names) == n, (kernel, names)
    assert {k["vgpr_spill_count"] for k in kernels} == {0}, kernels
    by_name = {k["name"]: k for k in kernels}
    n_aa = 0
    for name, k in by_name.items():
        print(name, k)
        if "Lb1EEE" in name and "k_hashgrid" in name:  # the AA flag is the last template argument
            sibling = by_name[name.replace("Lb1EEE", "Lb0EEE")]
            n_aa += 1
            assert k["sgpr_spill_count"] <= sibling["sgpr_spill_count"], (name, k, sibling)
            assert k["sgpr_spill_count"] == 0 or "k_hashgrid_bwdILb" in name, (name, k)
            assert k["private_segment_fixed_size"] == sibling["private_segment_fixed_size"], (name, k, sibling)
            assert k["vgpr_count"] <= 128, k  # (four waves per SIMD at the least)
    assert n_aa == 5


def test_host_layer_checks_its_arguments():
    P, cfg = hashfield.make_weights(0, {"log2_T": 10})
    x = torch.zeros(4, 3)
    res = torch.tensor(hashgrid.level_resolutions(cfg["L"], cfg["n_min"], cfg["n_max"]), dtype=torch.int32)
    rad = torch.zeros(4)
    with pytest.raises(RuntimeError, match="radius must not require grad"):
        hashgrid.hash_encode(x, P["hash.table"], res, cfg["log2_T"], radius=rad.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="radius must not require grad"):
        hashfield.forward(P, cfg, x, x, 4, radius=rad.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="radius must not require grad"):
        hashfield.forward_compacted(P, cfg, x, x, 4, radius=rad.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match=r"radius must be float32 of shape \(4,\)"):
        hashgrid.hash_encode(x, P["hash.table"], res, cfg["log2_T"], radius=torch.zeros(3))
    with pytest.raises(RuntimeError, match=r"radius must be float32 of shape \(4,\)"):
        hashgrid.hash_encode(x, P["hash.table"], res, cfg["log2_T"], radius=rad.double())
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match=r"outside \[0, 1\]"):
            hashgrid.hash_encode(x, P["hash.table"], res, cfg["log2_T"], radius=rad, w_min=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hashgrid.hash_encode(x, P["hash.table"], res, cfg["log2_T"], radius=rad)
    # the metric radius is measured against the smallest edge of the box
    Pb = dict(P, aabb=torch.tensor([[0.0, 0.0, 0.0], [2.0, 0.5, 1.0]]))
    assert torch.equal(hashfield._radius01(Pb, torch.tensor([0.25, 0.0])), torch.tensor([0.5, 0.0]))


def test_c_abi_checks_its_arguments_before_any_launch():
    """the new entry points refuse bad arguments with the library's error code and a message; nothing is launched (no GPU here)"""
    from lab4d_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(x=p, radius=p, table=p, res=p, g_out=p, S=4, L=16, log2_T=12, F=2, w_min=0.0, g_table=p, g_x=p)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.lab4d_hashgrid_forward_aa(a["x"], a["radius"], a["table"], a["res"], a["S"], a["L"], a["log2_T"], a["F"], a["w_min"], 1, a.get("out", p), None)

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.lab4d_hashgrid_backward_aa(a["x"], a["radius"], a["table"], a["res"], a["g_out"], a["S"], a["L"], a["log2_T"], a["F"], a["w_min"],
                                              a["g_table"], a["g_x"], None)

    def bwd16(**kw):
        a = dict(ok, **kw)
        return lib.lab4d_hashgrid_backward_f16_aa(a["x"], a["radius"], a["table"], a["res"], a["g_out"], a["S"], a["L"], a["log2_T"], a.get("l16", 3), a["w_min"],
                                                  a["g_table"], a.get("g16", p), a.get("amax", p), a["g_x"], None)

    for fn in (fwd, bwd, bwd16):
        for kw, msg in ((dict(radius=None), "null radius"), (dict(w_min=-0.5), "outside [0, 1]"), (dict(w_min=1.5), "outside [0, 1]"),
                        (dict(w_min=float("nan")), "outside [0, 1]"), (dict(w_min=float("inf")), "outside [0, 1]"), (dict(x=None), "null pointer"),
                        (dict(S=-1), "bad sizes"), (dict(log2_T=25), "bad sizes"), (dict(L=33), "bad sizes")):
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert msg in lib.lab4d_last_error().decode(), (fn.__name__, msg, lib.lab4d_last_error().decode())
        assert fn(S=0) == 0  # nothing to do: no launch
        assert fn(S=0, radius=None) == -1
    assert fwd(out=None) == -1 and "null output" in lib.lab4d_last_error().decode()
    assert bwd(g_table=None, g_x=None) == -1 and bwd(F=9) == -1
    assert bwd16(l16=17) == -1 and "first_f16_level" in lib.lab4d_last_error().decode()
    assert bwd16(g16=None) == -1
