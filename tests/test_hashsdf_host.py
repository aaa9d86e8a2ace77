"""The hash field's SDF gradient on the CPU: the twin of the kernels (tests/host_harness/hashsdf_host.cpp, the same
csrc/hashsdf_math.hpp functions) against float64 torch autograd over oracle/hashgrid_oracle.py (tests/hashsdf_checks.py: hash_encode,
the two Linears, autograd.grad(create_graph=True), a second autograd.grad).  The bound is 1e-4 relative L2 per tensor, the project's
fp32 bar; the GPU suite (tests/test_gpu_zzzzzzzhashsdf.py) holds the kernels to the same truth.  CPU only."""
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashsdf_checks as HC  # noqa: E402
import host_twin  # noqa: E402

import lab4d_amd.hashsdf  # noqa: E402,F401  (the feature under test: its host layer must import without a GPU)

S = 1025


@pytest.fixture(scope="module")
def host():
    return HC.build_host()


@pytest.mark.parametrize("name", sorted(HC.CONFIGS))
def test_twin_against_float64(host, name):
    """sdf, grad, every parameter gradient under random cotangents on both outputs, and the gradients of eikonal_loss.mean(): each within
    1e-4 relative L2 of float64.  (Rows 1..15 of the head gradient: asserted zero in the TRUTH only -- the twin, like the kernels, sees
    row 0 and the helper pads the rest; the product's rows are checked on the GPU, through the autograd slice.)"""
    P, cfg = HC.field(name)
    x, share = HC.points(P, cfg, S, seed=11)
    print("%s: dropped share %.4f" % (name, share))
    g_sdf, g_grad = HC.cotangents(S, 1)
    ref = HC.truth(P, cfg, x, g_sdf, g_grad)
    sdf, grad = HC.host_forward(host, P, cfg, x)
    errs = {"sdf": HC.rel_l2(sdf, ref["sdf"]), "grad": HC.rel_l2(grad, ref["grad"])}
    assert float(ref["grad"].norm(2, -1).mean()) > 0.1  # the gradient is of order 1, not 1e-3
    got = HC.host_backward(host, P, cfg, x, g_sdf, g_grad, n_rows=3)
    for k in HC.PARAMS:
        errs[k] = HC.rel_l2(got[k], ref[k])
    assert not ref["hash.geo.2.weight"][1:].any() and not ref["hash.geo.2.bias"][1:].any()
    inside = torch.ones(S, 1)
    eik = HC.truth(P, cfg, x, eikonal=True)
    got_e = HC.host_backward(host, P, cfg, x, None, HC.eikonal_cotangent(grad, inside), n_rows=3)
    loss = (grad.double().norm(2, -1, keepdim=True) - 1) ** 2
    errs["eikonal"] = HC.rel_l2(loss, eik["loss"])
    for k in HC.PARAMS[:4]:
        errs["eikonal " + k] = HC.rel_l2(got_e[k], eik[k])
    assert not got_e["hash.geo.2.bias"].any() and not eik["hash.geo.2.bias"].any()
    print(name, {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) < HC.TOL, errs
    # the partial rows: any resident grid gives the same dense gradients up to the order of the sums
    for n in (1, 512):
        other = HC.host_backward(host, P, cfg, x, g_sdf, g_grad, n_rows=n, want=HC.PARAMS[1:])
        assert all(HC.rel_l2(other[k], got[k]) < 1e-5 for k in HC.PARAMS[1:])


def specials(P, cfg):
    """x01 exactly 0 and 1 (3 points), outside the box (2), NaN (1), 64 identical points, 130 samples of a ray"""
    edge = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, 0.5, 1.0]])
    out = torch.tensor([[1.5, 0.5, 0.5], [0.5, -0.25, 0.5], [float("nan"), 0.5, 0.5]])
    same = torch.tensor([[0.3, 0.6, 0.2]]).repeat(64, 1)
    return edge, out, same, HC.ray_points(P, cfg)


def check_specials(P, cfg, fwd, bwd):
    """fwd(x) -> sdf (S,1), grad (S,3); bwd(x, g_sdf, g_grad) -> dict over PARAMS.  Shared with the GPU suite."""
    edge, out, same, ray = specials(P, cfg)
    # faces of the box: the weights are exactly 0 or 1 there, both sides pick the same (last) cell; and the ray
    for x in (edge, ray):
        g_sdf, g_grad = HC.cotangents(x.shape[0], 2)
        ref = HC.truth(P, cfg, x, g_sdf, g_grad)
        sdf, grad = fwd(x)
        assert HC.rel_l2(sdf, ref["sdf"]) < HC.TOL and HC.rel_l2(grad, ref["grad"]) < HC.TOL
        got = bwd(x, g_sdf, g_grad)
        for k in HC.PARAMS:
            assert HC.rel_l2(got[k], ref[k]) < HC.TOL, k
    # outside and NaN: sdf = w2 . relu(b1) + b2, grad exactly 0, the table and W1 get exact zeros, only the gs terms of b1, w2, b2 exist
    sdf, grad = fwd(out)
    w2, b2 = P["hash.geo.2.weight"][0].double(), P["hash.geo.2.bias"][0].double()
    want = float((w2 * torch.relu(P["hash.geo.0.bias"].double())).sum() + b2)
    assert float((sdf.double() - want).abs().max()) <= 1e-6 * max(1.0, abs(want)) and not grad.any()
    g_sdf, g_grad = HC.cotangents(3, 3)
    got = bwd(out, g_sdf, g_grad)
    assert not got["hash.table"].any() and not got["hash.geo.0.weight"].any()
    m = (P["hash.geo.0.bias"] > 0).double()
    gsum = float(g_sdf.double().sum())
    assert HC.rel_l2(got["hash.geo.0.bias"], gsum * m * w2) < 1e-6 and HC.rel_l2(got["hash.geo.2.bias"][:1], torch.tensor([gsum])) < 1e-6
    assert HC.rel_l2(got["hash.geo.2.weight"][0], gsum * torch.relu(P["hash.geo.0.bias"].double())) < 1e-6
    # 64 identical points (one wave: every table update of the wave falls into one run): 64 x the single point's gradients
    g1s, g1g = HC.cotangents(1, 4)
    one = bwd(same[:1], g1s, g1g)
    all64 = bwd(same, g1s.repeat(64, 1), g1g.repeat(64, 1))
    for k in HC.PARAMS:
        assert HC.rel_l2(all64[k], 64 * one[k].double()) < 1e-5, k
    s64, gr64 = fwd(same)
    assert bool((s64 == s64[0]).all()) and bool((gr64 == gr64[0]).all())


@pytest.mark.parametrize("name", sorted(HC.CONFIGS))
def test_special_points(host, name):
    P, cfg = HC.field(name)
    check_specials(P, cfg, lambda x: HC.host_forward(host, P, cfg, x), lambda x, a, b: HC.host_backward(host, P, cfg, x, a, b, n_rows=3))


def test_zero_table_gives_loss_one_and_finite_gradients(host):
    P, cfg = HC.field("a", zero_table=True)
    x, _ = HC.points(P, cfg, 257, seed=5)
    sdf, grad = HC.host_forward(host, P, cfg, x)
    assert not grad.any()
    loss = (grad.norm(2, -1, keepdim=True) - 1) ** 2
    assert bool((loss == 1).all())
    got = HC.host_backward(host, P, cfg, x, None, HC.eikonal_cotangent(grad, torch.ones(257, 1)), n_rows=3)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


def test_twin_runs_clean_under_the_sanitizers():
    """the stand-alone program over the special points of the rules, AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU"""
    r = subprocess.run([host_twin.sanitized_main("hashsdf")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hashsdf_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_no_hashsdf_kernel_uses_scratch(tmp_path):
    """csrc/hashsdf.hip compiled for gfx950 as the build does: the code-object metadata of the three kernels (the forward and the adjoint
    once per F in 1, 2, 4, 8, and the reduce) reports no private segment and no spills."""
    kernels = host_twin.kernel_metadata("hashsdf.hip", tmp_path)
    names = [k["name"] for k in kernels]
    assert len(names) == 9, names
    for kernel, n in (("k_hashsdf_fwd", 4), ("k_hashsdf_bwd", 4), ("k_hashsdf_reduce", 1)):
        assert sum(kernel in x for x in names) == n, (kernel, names)
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
    # three waves per SIMD: 512 / 3 registers rounded down to the allocation granule of 8 = 168.  The empty-asm pins of hashsdf_math.hpp hold
    # the allocation there; undone by a compiler, the kernels fall back to one wave per SIMD (256 VGPRs + AGPR copies) without spilling
    assert max(k["vgpr_count"] for k in kernels) <= 168, kernels  # (the unified count: AGPRs included)
    assert all(k["agpr_count"] == 0 for k in kernels), kernels


def test_host_layer_checks_its_arguments():
    from lab4d_amd import hashfield, hashsdf
    P, cfg = HC.field("a", unit_box=False)
    x = torch.zeros(4, 3)
    res = torch.tensor(HC.res_list(cfg), dtype=torch.int32)
    net = (P["hash.geo.0.weight"], P["hash.geo.0.bias"], P["hash.geo.2.weight"][0], P["hash.geo.2.bias"][:1])
    with pytest.raises(RuntimeError, match="must not require grad"):
        hashfield.sdf_gradient(P, cfg, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="must not require grad"):
        hashfield.eikonal_loss(P, cfg, x.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="must not require grad"):
        hashsdf.sdf_grad01(x.clone().requires_grad_(True), P["hash.table"], res, cfg["log2_T"], *net)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hashfield.sdf_gradient(P, cfg, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hashfield.normals(P, cfg, x)
    with pytest.raises(RuntimeError, match=r"x01 must be float32 \(S, 3\)"):
        hashsdf.sdf_grad01(x.double(), P["hash.table"], res, cfg["log2_T"], *net)
    with pytest.raises(RuntimeError, match=r"L \* F = 32"):
        hashsdf.sdf_grad01(x, P["hash.table"][:8], res[:8], cfg["log2_T"], *net)
    with pytest.raises(RuntimeError, match="2\\^log2_T rows"):
        hashsdf.sdf_grad01(x, P["hash.table"], res, cfg["log2_T"] + 1, *net)
    with pytest.raises(RuntimeError, match=r"res must be int32"):
        hashsdf.sdf_grad01(x, P["hash.table"], res.long(), cfg["log2_T"], *net)
    with pytest.raises(RuntimeError, match=r"w2 must be float32 \(64,\)"):
        hashsdf.sdf_grad01(x, P["hash.table"], res, cfg["log2_T"], net[0], net[1], P["hash.geo.2.weight"], net[3])
    with pytest.raises(RuntimeError, match=r"work_rows = 0 outside \[1, 512\]"):
        hashsdf.sdf_grad01(x, P["hash.table"], res, cfg["log2_T"], *net, work_rows=0)
    with pytest.raises(NotImplementedError, match="L\\*F = 32"):
        hashfield.sdf_gradient(P, dict(cfg, L=8), x)
    assert hashsdf.ROW == 2048 + 64 + 64 + 1 and hashsdf.MAX_ROWS == 512


def test_c_abi_checks_its_arguments_before_any_launch():
    """the entry points refuse bad arguments with the library's error code and a message; nothing is launched (no GPU here)"""
    import ctypes
    from lab4d_amd import _lib
    lib = _lib.lib()
    from lab4d_amd import hashsdf
    header = open(os.path.join(_lib.INCLUDE, "lab4d_hashsdf.h")).read()
    assert int(re.search(r"#define LAB4D_HASHSDF_WORK_ROWS (\d+)", header).group(1)) == hashsdf.MAX_ROWS
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(x01=p, table=p, res=p, S=4, L=16, log2_T=12, F=2, W1=p, b1=p, w2=p, b2=p)

    def fwd(**kw):
        a = dict(dict(ok, sdf=p, grad01=p), **kw)
        return lib.lab4d_hashsdf_forward(a["x01"], a["table"], a["res"], a["S"], a["L"], a["log2_T"], a["F"], a["W1"], a["b1"], a["w2"], a["b2"], a["sdf"],
                                         a["grad01"], None)

    def bwd(**kw):
        a = dict(dict(ok, g_sdf=p, g_grad01=p, g_table=p, g_W1=p, g_b1=p, g_w2=p, g_b2=p, work=p, n_work_rows=3), **kw)
        return lib.lab4d_hashsdf_backward(a["x01"], a["table"], a["res"], a["S"], a["L"], a["log2_T"], a["F"], a["W1"], a["b1"], a["w2"], a["b2"], a["g_sdf"],
                                          a["g_grad01"], a["g_table"], a["g_W1"], a["g_b1"], a["g_w2"], a["g_b2"], a["work"], a["n_work_rows"], None)

    cases = [(fwd, dict(L=8), "L = 8, F = 2"), (fwd, dict(L=2, F=16), "F = 16"), (fwd, dict(log2_T=3), "log2_T = 3"), (fwd, dict(log2_T=25), "log2_T = 25"),
             (fwd, dict(S=-1), "negative"), (fwd, dict(x01=None), "null pointer (x01"), (fwd, dict(w2=None), "null pointer (W1"),
             (fwd, dict(sdf=None), "null pointer (sdf)"), (bwd, dict(F=3), "L = 16, F = 3"), (bwd, dict(g_sdf=None, g_grad01=None), "at least one cotangent"),
             (bwd, dict(g_table=None, g_W1=None, g_b1=None, g_w2=None, g_b2=None), "no gradient asked for"), (bwd, dict(work=None), "work buffer"),
             (bwd, dict(n_work_rows=0), "n_work_rows = 0"), (bwd, dict(n_work_rows=513), "n_work_rows = 513")]
    for fn, kw, msg in cases:
        assert fn(**kw) == -1, (kw, msg)
        assert msg in lib.lab4d_last_error().decode(), (msg, lib.lab4d_last_error().decode())
