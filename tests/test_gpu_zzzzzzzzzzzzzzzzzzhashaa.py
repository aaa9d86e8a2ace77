"""The footprint-weighted hash encoding on the device (the AA instantiations of csrc/hashgrid.hip through hashgrid.hash_encode(radius=...),
hashfield.forward / forward_compacted(radius=...), hashfield.sample_radius and render_packed / render_packed_cone(footprint=...)).

The truth is the float64 definition of tests/hashaa_checks.py; the yardstick is the CPU twin (tests/host_harness/hashaa/hashaa_host.cpp: the same fp32
formula, differing from the device in erff and in contraction only): its error against float64 is computed here, at run time, and the device's
must lie within 4 x that (a 2-ulp erff, the order of the atomics).  out and g_x are per-sample quantities -- a sample's value does not depend
on the rows around it -- so every size S is a prefix of one set of 1000 rows and the twin's error over all of them (its largest entry error) is
the yardstick at every S: three values at S = 1 measure no noise level.  The table gradient depends on S: the twin's relative L2 per level at
that S, and 1e-6 where it is smaller.  tests/test_hashaa_host.py pins the twin itself."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conemarch_checks as CC  # noqa: E402
import hashaa_checks as AC  # noqa: E402

from lab4d_amd import hashfield, hashgrid, mlp, occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(None)
def device_table(name):
    return dev(AC.table(name)), torch.tensor(AC.res_list(name), dtype=torch.int32, device=DEV)


def encode(name, x, rad, w_min, inside_only, g_out=None, f16_from=None, want_table=True):
    """hash_encode on the device -> out, or (out, g_table, g_x) under the cotangent g_out; rad None: the unweighted kernels"""
    tab, res = device_table(name)
    log2_T = AC.CONFIGS[name][2]
    xd, td = dev(x).requires_grad_(g_out is not None), tab.clone().requires_grad_(g_out is not None and want_table)
    out = hashgrid.hash_encode(xd, td, res, log2_T, inside_only=inside_only, f16_from=f16_from, radius=None if rad is None else dev(rad), w_min=w_min)
    if g_out is None:
        return out.detach()
    g_x, g_table = torch.autograd.grad((out * dev(g_out)).sum(), [xd, td])
    return out.detach(), g_table, g_x


def within(err, yard, what):
    print("%s: device %.3e, twin %.3e, ratio %s" % (what, err, yard, "%.2f" % (err / yard) if yard > 0 else "-"))
    assert err <= AC.FACTOR * yard, (what, err, yard)


@pytest.mark.parametrize("inside_only", [False, True])
@pytest.mark.parametrize("w_min", AC.W_MINS)
@pytest.mark.parametrize("pattern", AC.PATTERNS)
@pytest.mark.parametrize("name", sorted(AC.CONFIGS))
def test_kernels_against_float64_within_four_times_the_twin(name, pattern, w_min, inside_only):
    """cases 1, 2, 4, 5: every size, every radius pattern, both cuts, the sample-major forward with and without the box test and the backward.
    radius = inf: the twin's error is zero, so the device's outputs are exactly zero"""
    c = AC.case(name, pattern, w_min, inside_only)
    for S in AC.SIZES:
        x, rad, g = c["x"][:S], c["radius"][:S], c["g_out"][:S]
        out, g_table, g_x = encode(name, x, rad, w_min, inside_only, g)
        out, g_table, g_x = out.cpu().numpy(), g_table.cpu().numpy(), g_x.cpu().numpy()
        what = "%s %s w_min %g inside %d S %d" % (name, pattern, w_min, inside_only, S)
        within(AC.max_abs(out, c["ref_out"][:S]), c["yard_out"], what + " out")
        within(AC.max_abs(g_x, c["ref_gx"][:S]), c["yard_gx"], what + " g_x")
        assert (out[c["ref_out"][:S] == 0] == 0).all(), what  # a zero weight, a point outside the box: exact zeros
        ref, _, twin_err = AC.table_gradients(c, S)
        err, bound = AC.level_rel_l2(g_table, ref), AC.table_bound(twin_err)
        print(what + " g_table per level: device %s twin %s" % (np.array2string(err, precision=2), np.array2string(twin_err, precision=2)))
        assert (err <= bound).all(), (what, err, bound)
        assert (g_table[(ref == 0).all((1, 2))] == 0).all(), what  # a level nobody weighs: untouched
        if pattern == "inf":
            assert not out.any() and not g_x.any() and not g_table.any()


@pytest.mark.parametrize("name,pattern,inside_only", [(n, p, i) for n in sorted(AC.CONFIGS) for p, i in (("loguniform", True), ("raylike", True), ("loguniform", False))])
def test_forward_on_both_sides_of_the_level_major_dispatch(name, pattern, inside_only):
    """case 1, S = 65535 and 65536: the inside-only forward changes to the level-major kernel at 65536 (a thread whose weight is 0 writes zeros
    without touching the slab); without the box test both sizes run the sample-major kernel"""
    w_min = 1.0 / 256
    c = AC.case(name, pattern, w_min, inside_only, n=AC.BIG)
    for S in (AC.BIG - 1, AC.BIG):
        out = encode(name, c["x"][:S], c["radius"][:S], w_min, inside_only).cpu().numpy()
        what = "%s %s inside %d S %d" % (name, pattern, inside_only, S)
        within(AC.max_abs(out, c["ref_out"][:S]), c["yard_out"], what + " out")
        assert (out[c["ref_out"][:S] == 0] == 0).all(), what
        zero = encode(name, c["x"][:S], np.zeros(S, np.float32), w_min, inside_only)
        assert torch.equal(zero, encode(name, c["x"][:S], None, 0.0, inside_only)), what  # radius 0: the unweighted kernel of the same branch, bit for bit
    assert (c["ref_out"] == 0).mean() > 0.02


@pytest.mark.parametrize("inside_only", [False, True])
@pytest.mark.parametrize("name", sorted(AC.CONFIGS))
def test_radius_zero_equals_the_unweighted_kernels(name, inside_only):
    """case 3: out and g_x bit for bit; the table gradient to 1e-6 relative L2, "equal up to the order of the atomics\""""
    c = AC.case(name, "zero", 0.0, inside_only)
    for S in AC.SIZES:
        x, g = c["x"][:S], c["g_out"][:S]
        plain = encode(name, x, None, 0.0, inside_only, g)
        for w_min in (0.0, 1.0 / 256):
            got = encode(name, x, np.zeros(S, np.float32), w_min, inside_only, g)
            assert torch.equal(got[0], plain[0]) and torch.equal(got[2], plain[2]), (name, S, w_min)
            e = float((got[1] - plain[1]).norm() / plain[1].norm().clamp_min(1e-30))
            assert e <= AC.TABLE_FLOOR, (name, S, w_min, e)
        negative = encode(name, x, np.full(S, -1.0, np.float32), 0.0, inside_only)
        assert torch.equal(negative, plain[0])


@pytest.mark.parametrize("w_min", AC.W_MINS)
@pytest.mark.parametrize("pattern", AC.MIXED)
@pytest.mark.parametrize("name", sorted(AC.CONFIGS))
def test_kernel_equals_the_composition_on_the_device(name, pattern, w_min):
    """case 6: hash_encode(x, radius=r, w_min=m) against hash_encode(x) * level_weights(r, res, m), both on the device, within 4 x the twin's
    error; exactly zero where level_weights is zero"""
    c = AC.case(name, pattern, w_min, True)
    F = AC.CONFIGS[name][1]
    _, res = device_table(name)
    for S in AC.SIZES:
        x, rad = c["x"][:S], c["radius"][:S]
        w = hashgrid.level_weights(dev(rad), res, w_min)
        assert tuple(w.shape) == (S, len(c["res"]))
        composed = encode(name, x, None, 0.0, True) * w.repeat_interleave(F, -1)
        out = encode(name, x, rad, w_min, True)
        within(float((out - composed).abs().max()), c["yard_out"], "%s %s w_min %g S %d composition" % (name, pattern, w_min, S))
        assert bool((out[w.repeat_interleave(F, -1) == 0] == 0).all())
    if w_min > 0:
        assert 0.01 < float((w == 0).float().mean()) < 0.99


@pytest.mark.parametrize("pattern", AC.MIXED)
def test_packed_fp16_table_gradient_with_weights(pattern):
    """case 7: f16_from = the first hashed level against the fp32 path -- dense levels < 1e-6, hashed levels < 1e-3 relative L2 (the bounds of
    tests/test_gpu_zzhashgrid.py's packed-fp16 test), finite, g_x as there; a second call reuses the cleared scratch and meets the same bounds"""
    name, w_min = "a", 1.0 / 256
    c = AC.case(name, pattern, w_min, False)
    l16 = hashgrid.first_hashed_level(c["res"], AC.CONFIGS[name][2])
    assert 0 < l16 < len(c["res"])
    _, g32, gx32 = encode(name, c["x"], c["radius"], w_min, False, c["g_out"])
    first = None
    for call in range(2):
        _, g16, gx16 = encode(name, c["x"], c["radius"], w_min, False, c["g_out"], f16_from=l16)
        if first is None:
            first = g16
        else:  # the same result up to the order of the atomics: a scratch word left uncleared would add call 0's sum to call 1's
            again = float((g16[l16:] - first[l16:]).norm() / first[l16:].norm())
            print("%s call 1 against call 0, hashed levels: %.2e" % (pattern, again))
            assert again < 1e-3, again
        dense = float((g16[:l16] - g32[:l16]).norm() / g32[:l16].norm())
        hashed = float((g16[l16:] - g32[l16:]).norm() / g32[l16:].norm())
        print("%s call %d: dense %.2e hashed %.2e" % (pattern, call, dense, hashed))
        assert dense < 1e-6 and hashed < 1e-3, (call, dense, hashed)
        assert bool(torch.isfinite(g16).all())
        assert float((gx32 - gx16).abs().max()) <= 1e-5 * float(gx32.abs().max())
    assert float(g32[l16:].norm()) > 0


# ---------------------------------------------------------------------------------------------------
# the field
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def field():
    cfg = {"L": 16, "F": 2, "log2_T": 14, "n_min": 16, "n_max": 512}
    P, cfg = hashfield.make_weights(3, cfg, sdf_bias=0.01)
    P["hash.table"] = P["hash.table"] * 3e3  # features of order 0.3 so that the nets see a signal (tests/test_gpu_zzhashgrid.py's field)
    return P, cfg


@pytest.mark.parametrize("w_min", AC.W_MINS)
def test_weighted_field_matches_its_torch_restatement(w_min):
    """case 8: hashfield.forward(radius=...) and forward_compacted(radius=..., cap=...) at fp32 against AC.field_reference on the CPU, to the
    bounds of test_hash_field_matches_the_oracle[f32] (2e-4 on values, 2e-3 on gradients); S = 1000, half of the points outside the box;
    forward_compacted equals forward sample for sample"""
    P, cfg = field()
    g = torch.Generator().manual_seed(5)
    S = 1000
    xyz = (torch.rand(S, 3, generator=g) * 2 - 1) * 0.15
    dirs = torch.nn.functional.normalize(torch.randn(S, 3, generator=g), dim=-1)
    rad = torch.from_numpy(AC.radius("loguniform", S, seed=9)) * 0.24  # metric: log-uniform in [1e-5, 10] box edges
    names = [k for k in P if k != "aabb"]
    cw = [torch.randn(S, 3, generator=g), torch.randn(S, 1, generator=g)]
    assert 300 < int((xyz.abs() <= 0.12).all(-1).sum()) < 700

    def run(fwd, where):
        Pl = {k: (v.to(where).clone().requires_grad_(True) if k in names else v.to(where)) for k, v in P.items()}
        x = xyz.to(where).clone().requires_grad_(True)
        rgb, dens = fwd(Pl, x, dirs.to(where), rad.to(where))
        loss = (rgb * cw[0].to(where)).sum() + (dens * cw[1].to(where)).sum() * 1e-2
        gs = torch.autograd.grad(loss, [Pl[k] for k in names] + [x])
        return rgb.detach(), dens.detach(), dict(zip(names + ["xyz"], gs))

    rr, rd, rg = run(lambda Pl, x, d, r: AC.field_reference(Pl, cfg, x, d, r, w_min), "cpu")
    _, ud, _ = run(lambda Pl, x, d, r: AC.field_reference(Pl, cfg, x, d, torch.zeros_like(r), w_min), "cpu")
    assert float((ud - rd).abs().max()) > 0.1  # the weights matter to the result (the density reaches 4)
    dr, dd, dg = run(lambda Pl, x, d, r: hashfield.forward(Pl, cfg, x, d, spf=S, prec=mlp.PREC_F32, radius=r, w_min=w_min), DEV)
    rel = lambda a, b: float((a.detach().cpu() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-12))
    errs = {"rgb": rel(dr, rr), "density": rel(dd, rd)}
    gerrs = {k: rel(dg[k], rg[k]) for k in names + ["xyz"]}
    print("weighted field against torch:", errs, gerrs)
    assert max(errs.values()) < 2e-4, errs
    assert max(gerrs.values()) < 2e-3, gerrs
    cr, cd, cg = run(lambda Pl, x, d, r: hashfield.forward_compacted(Pl, cfg, x, d, 1024, prec=mlp.PREC_F32, radius=r, w_min=w_min)[:2], DEV)
    assert torch.equal(cr, dr) and torch.equal(cd, dd)
    for k in names + ["xyz"]:
        e = float((cg[k] - dg[k]).norm() / dg[k].norm().clamp_min(1e-20))
        assert e < 1e-5, (k, e)  # (the bound of test_compacted_field_equals_the_full_field[f32]: equal up to the summation order)


# ---------------------------------------------------------------------------------------------------
# rendering
# ---------------------------------------------------------------------------------------------------
K_R, G_R, R_R, CONE_R, DT_MIN_R, DT_MAX_R, K_MAX_R, FOOTPRINT = 2, 8, 65, 0.05, 0.002, 0.02, 200, 0.05


@functools.lru_cache(None)
def scene():
    """the field on the outermost box of a K = 2, G = 8 cascade (every bit set) and the first 65 rays of tests/conemarch_checks.py's ray set
    (its special rays -- non-finite inputs, misses, a zero direction -- among them)"""
    P, cfg = field()
    base = (P["aabb"] / 2).numpy()
    aabbs = CC.cascade_boxes(K_R, base)
    assert np.array_equal(aabbs[K_R - 1], P["aabb"].numpy().reshape(6))
    o, d, tr, _ = CC.ray_set(aabbs)
    casc = occgrid.OccupancyCascade(dev(base), K=K_R, G=G_R)
    Pd = {k: v.to(DEV) for k, v in P.items()}
    return Pd, cfg, casc, dev(o[:R_R]), dev(d[:R_R]), dev(tr[:R_R]), R_R * K_MAX_R


def test_render_packed_cone_with_a_footprint():
    """case 9: footprint = 0 is the unweighted render bit for bit; footprint = f is packed.composite of forward(radius = sample_radius(...)) on
    the same march_cone list bit for bit; sample_radius is t |dir| f on the kept rows and 0 on the parked ones; the refusals"""
    Pd, cfg, casc, o, d, tr, cap = scene()
    args = (Pd, cfg, casc, o, d, tr, CONE_R, DT_MIN_R, DT_MAX_R, cap)
    with torch.no_grad():
        plain = hashfield.render_packed_cone(*args, k_max=K_MAX_R)
        zero = hashfield.render_packed_cone(*args, k_max=K_MAX_R, footprint=0.0)
        assert len(zero) == 5 and all(torch.equal(a, b) for a, b in zip(plain, zero))
        got = hashfield.render_packed_cone(*args, k_max=K_MAX_R, footprint=FOOTPRINT, with_distortion=True)
        rays = packed.march_cone(casc, o, d, tr, CONE_R, DT_MIN_R, DT_MAX_R, cap, k_max=K_MAX_R)
        n = int(rays.total)
        assert 1000 < n < cap and int(got[3]) == n and not bool(got[4])
        rad = hashfield.sample_radius(rays, d, FOOTPRINT)
        assert tuple(rad.shape) == (cap,) and rad.dtype == torch.float32
        assert bool((rays.ray_idx[n:] == -1).all()) and bool((rad[n:] == 0).all()) and bool((rad[:n] != 0).all())
        assert torch.equal(rad[:n], rays.t[:n] * d.norm(2, -1)[rays.ray_idx[:n].long()] * FOOTPRINT)
        rgb_s, dens_s = hashfield.forward(Pd, cfg, rays.xyz, rays.dirs, spf=cap, radius=rad, w_min=1.0 / 256)
        rendered, mask = packed.composite(dens_s, rays.deltas, {"rgb": rgb_s, "depth": rays.t[:, None]}, rays)
        assert torch.equal(got[0], rendered["rgb"]) and torch.equal(got[1], mask) and torch.equal(got[2], rendered["depth"])
        assert torch.equal(got[5], packed.distortion(dens_s, rays.deltas, rays.t, rays.steps, rays)[:, None])
        assert float((got[0] - plain[0]).abs().max()) > 1e-4  # the footprint changes the picture
        w = hashgrid.level_weights(rad[:n] / 0.24, hashfield.resolutions(cfg, DEV), 1.0 / 256)
        assert float((w[:, -1] < 0.5).float().mean()) > 0.5 and float(w[:, 0].min()) > 0  # the finest level damped, the coarsest alive
        # the fixed-step march takes the same arguments
        grid = casc.level_grid(K_R - 1)
        p_args = (Pd, cfg, grid, o, d, tr, DT_MAX_R, cap)
        p_plain, p_zero = hashfield.render_packed(*p_args, k_max=K_MAX_R), hashfield.render_packed(*p_args, k_max=K_MAX_R, footprint=0.0)
        assert all(torch.equal(a, b) for a, b in zip(p_plain, p_zero))
        p_got = hashfield.render_packed(*p_args, k_max=K_MAX_R, footprint=FOOTPRINT)
        p_rays = packed.march(grid, o, d, tr, DT_MAX_R, cap, k_max=K_MAX_R)
        p_rgb, p_dens = hashfield.forward(Pd, cfg, p_rays.xyz, p_rays.dirs, spf=cap, radius=hashfield.sample_radius(p_rays, d, FOOTPRINT), w_min=1.0 / 256)
        p_rendered, p_mask = packed.composite(p_dens, p_rays.deltas, {"rgb": p_rgb, "depth": p_rays.t[:, None]}, p_rays)
        assert int(p_got[3]) > 500 and torch.equal(p_got[0], p_rendered["rgb"]) and torch.equal(p_got[1], p_mask)
    for render, a in ((hashfield.render_packed_cone, args), (hashfield.render_packed, p_args)):
        with pytest.raises(NotImplementedError, match="footprint together with with_normal=True"):
            render(*a, k_max=K_MAX_R, footprint=FOOTPRINT, with_normal=True)
    bad = rad.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="radius must not require grad"):
        hashfield.forward(Pd, cfg, rays.xyz, rays.dirs, spf=cap, radius=bad)
    with pytest.raises(RuntimeError, match="radius must not require grad"):
        hashfield.forward_compacted(Pd, cfg, rays.xyz, rays.dirs, cap, radius=bad)
    with pytest.raises(RuntimeError, match="radius must not require grad"):
        hashgrid.hash_encode(rays.xyz, Pd["hash.table"], hashfield.resolutions(cfg, DEV), cfg["log2_T"], radius=bad)


def test_gradients_reach_the_parameters_through_a_weighted_render():
    """the weighted render trains: finite, non-zero gradients in the table, every Linear and logibeta; no table gradient at the levels that
    every kept row cuts"""
    Pd, cfg, casc, o, d, tr, cap = scene()
    tr = tr.clone()
    tr[:, 0] = tr[:, 0].clamp_min(0.5)  # no row close to its camera: with footprint 2 the finest level is cut on every kept row (asserted below)
    names = [k for k in Pd if k != "aabb"]
    Pl = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in Pd.items()}
    rgb, mask, depth, _, _ = hashfield.render_packed_cone(Pl, cfg, casc, o, d, tr, CONE_R, DT_MIN_R, DT_MAX_R, cap, k_max=K_MAX_R, footprint=2.0)
    grads = dict(zip(names, torch.autograd.grad(rgb.sum() + mask.sum() + depth.sum(), [Pl[k] for k in names])))
    assert all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0 for v in grads.values())
    rays = packed.march_cone(casc, o, d, tr, CONE_R, DT_MIN_R, DT_MAX_R, cap, k_max=K_MAX_R)
    w = hashgrid.level_weights(hashfield.sample_radius(rays, d, 2.0)[:int(rays.total)] / 0.24, hashfield.resolutions(cfg, DEV), 1.0 / 256)
    dead = (w == 0).all(0)
    assert int(rays.total) > 500 and bool(dead[-1]) and not bool(dead[0])
    assert not bool(grads["hash.table"][dead].any()) and bool(grads["hash.table"][~dead].any())


def test_weighted_forward_is_capturable():
    """case 10: one capture and replay of the weighted forward (one stream, no parallel branches) equals eager bit for bit"""
    name, w_min = "a", 1.0 / 256
    c = AC.case(name, "raylike", w_min, True)
    tab, res = device_table(name)
    x, rad = dev(c["x"]), dev(c["radius"])
    eager = hashgrid.hash_encode(x, tab, res, AC.CONFIGS[name][2], inside_only=True, radius=rad, w_min=w_min)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):  # one stream, no parallel branches
        out = hashgrid.hash_encode(x, tab, res, AC.CONFIGS[name][2], inside_only=True, radius=rad, w_min=w_min)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and float(eager.abs().max()) > 0.05
    rad.copy_(dev(AC.radius("alternating", AC.N_ROWS)))  # the graph reads the radius at replay
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, hashgrid.hash_encode(x, tab, res, AC.CONFIGS[name][2], inside_only=True, radius=rad, w_min=w_min))
