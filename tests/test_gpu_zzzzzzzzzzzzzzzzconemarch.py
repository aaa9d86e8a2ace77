"""Cascaded occupancy grids and the cone-stepped packed march on the device (csrc/conemarch.hip through occgrid.OccupancyCascade,
packed.march_cone and hashfield.render_packed_cone): the kernels against the CPU twin (tests/host_harness/conemarch/conemarch_host.cpp) WORD FOR
WORD, the cascade's update against the numpy rule, render_packed_cone against torch on the emitted rows, the list through prune / resample /
merge, graph capture.  tests/test_conemarch_host.py pins the twin itself."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conemarch_checks as CC  # noqa: E402
import distort_checks as DC  # noqa: E402
import occgrid_checks as OC  # noqa: E402
import packed_checks as PC  # noqa: E402

from lab4d_amd import occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_BOUND = 1e-5  # relative L2 per tensor: the bound of tests/test_gpu_zzzzzpacked.py::test_render_packed_equals_the_dense_lattice_through_the_merged_path


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def new_cascade(K, G, occ=None, base=OC.AABB, **kw):
    casc = occgrid.OccupancyCascade(dev(base), K=K, G=G, **kw)
    assert np.array_equal(casc.aabbs.cpu().numpy(), CC.cascade_boxes(K, base))  # float64, rounded once: the boxes of the twin's tests
    if occ is not None:
        casc.bits.copy_(dev(CC.pack_levels(occ).view(np.int32)))
    return casc


def as_dict(rays):
    out = {k: getattr(rays, k).cpu().numpy() for k in CC.FIELDS + ("ray_idx", "level", "ray_start", "ray_count")}
    assert rays.total.dtype == torch.int32 and rays.overflow.dtype == torch.bool
    out.update(total=int(rays.total), overflow=bool(rays.overflow), R=rays.R, cap=rays.cap)
    return out


@pytest.mark.parametrize("K,G", [(1, 4), (1, 32), (4, 4), (4, 32)])
def test_march_kernels_equal_the_cpu_twin_word_for_word(K, G):
    """every R in 1 / 63 / 64 / 65 / 1025 (the wave and block edges of the count pass) with every k_max in 1 / 64 / 65 / 200, the cone angles
    in turn, and the capacities total, total - 1, a cut inside a ray and 0; then an all-empty cascade"""
    lib = CC.build_host()
    aabbs = CC.cascade_boxes(K)
    o, d, tr, _ = CC.ray_set(aabbs)
    occ = CC.cascade_occupancy(K, G, 3)
    bits = CC.pack_levels(occ)
    casc = new_cascade(K, G, occ)
    n_total, i = 0, 0
    for R in (1, 63, 64, 65, 1025):
        od, dd, td = dev(o[:R]), dev(d[:R]), dev(tr[:R])
        for k_max in (1, 64, 65, 200):
            cone = CC.CONES[i % 3]
            i += 1
            full = CC.host_march(lib, o[:R], d[:R], tr[:R], aabbs, bits, G, cone, CC.DT_MIN, CC.DT_MAX, k_max)
            total = full["total"]
            inside = next((int(full["ray_start"][r]) + 1 for r in range(R) if full["count"][r] >= 2), 0)
            for cap in sorted({total, max(total - 1, 0), inside, 0}):
                ref = full if cap == total else CC.host_march(lib, o[:R], d[:R], tr[:R], aabbs, bits, G, cone, CC.DT_MIN, CC.DT_MAX, k_max, cap=cap)
                got = packed.march_cone(casc, od, dd, td, cone, CC.DT_MIN, CC.DT_MAX, cap, k_max=k_max)
                CC.assert_same(as_dict(got), ref, (K, G, R, k_max, cone, cap))
            n_total += total
    assert n_total > 5000
    empty = CC.cascade_occupancy(K, G, 0, "empty")
    got = packed.march_cone(new_cascade(K, G, empty), dev(o[:65]), dev(d[:65]), dev(tr[:65]), 0.05, CC.DT_MIN, CC.DT_MAX, 7, k_max=64)
    CC.assert_same(as_dict(got), CC.host_march(lib, o[:65], d[:65], tr[:65], aabbs, CC.pack_levels(empty), G, 0.05, CC.DT_MIN, CC.DT_MAX, 64, cap=7), "empty")
    assert int(got.total) == 0 and not bool(got.overflow) and bool((got.ray_idx == -1).all()) and bool((got.level == -1).all())
    got = packed.march_cone(casc, dev(o[:0]), dev(d[:0]), dev(tr[:0]), 0.05, CC.DT_MIN, CC.DT_MAX, 7, k_max=64)
    CC.assert_same(as_dict(got), CC.host_march(lib, o[:0], d[:0], tr[:0], aabbs, bits, G, 0.05, CC.DT_MIN, CC.DT_MAX, 64, cap=7), "no rays")


@pytest.mark.parametrize("K,G", [(1, 32), (4, 4), (4, 32)])
def test_cascade_mask_equals_the_cpu_twin(K, G):
    lib = CC.build_host()
    aabbs = CC.cascade_boxes(K)
    occ = CC.cascade_occupancy(K, G, 11)
    casc = new_cascade(K, G, occ)
    pts, delta = CC.mask_points(4097, 7, aabbs)
    delta[:K], delta[K], delta[K + 1], delta[K + 2] = CC.f32_edges(aabbs, G), 0.0, np.nan, np.inf
    for dl in (delta, None):
        mask, level = casc.mask(dev(pts), None if dl is None else dev(dl))
        want_mask, want_level = CC.host_cascade_mask(lib, pts, dl, aabbs, CC.pack_levels(occ), G)
        assert mask.dtype == torch.uint8 and level.dtype == torch.int32
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(level.cpu().numpy(), want_level)
        assert 0 < int(mask.sum()) < 4097
    if K == 1:  # one level: the plain grid's mask
        assert torch.equal(mask, casc.level_grid(0).mask(dev(pts)))


@pytest.mark.parametrize("G", [32, 6])
def test_cascade_update_equals_the_numpy_rule_and_keeps_the_parents(G):
    K, decay, thresh = 3, 0.95, 0.01
    casc = new_cascade(K, G, decay=decay, thresh=thresh)
    assert bool((casc.ema == float("inf")).all()) and casc.n_occupied.tolist() == [G ** 3] * K and tuple(casc.cell_centers().shape) == (K, G ** 3, 3)
    assert np.array_equal(np.stack([OC.unpack(w, G) for w in casc.bits.cpu().numpy().view(np.uint32)]), np.ones((K, G, G, G), bool))
    ema = CC.np_cascade_new(K, G)
    for step in range(3):
        dens = CC.cascade_density(K, G, 100 * step + G)
        if step == 2:
            dens[1] = 0.0
        want = CC.np_cascade_update(ema, dens, K, G, decay, thresh)
        assert casc.update(dev(dens)) is casc
        got = np.stack([OC.unpack(w, G) for w in casc.bits.cpu().numpy().view(np.uint32)])
        assert np.array_equal(got, want), step
        assert casc.n_occupied.tolist() == [int(w.sum()) for w in want]
        assert np.array_equal(casc.ema.cpu().numpy(), ema)
        assert CC.parents_hold(got) and 0 < got[0].sum() < G ** 3
    # a level's grid shares the cascade's storage, and its centres are the level's
    g1 = casc.level_grid(1)
    assert g1.bits.data_ptr() == casc.bits[1].data_ptr() and g1.ema.data_ptr() == casc.ema[1].data_ptr() and g1.n_occupied.data_ptr() == casc.n_occupied[1:].data_ptr()
    assert torch.equal(g1.cell_centers(), casc.cell_centers()[1]) and torch.equal(g1.aabb.reshape(6), casc.aabbs[1])
    g1.update(torch.zeros(G ** 3, device=DEV))  # what a grid's own call writes is the cascade's
    assert np.array_equal(casc.ema[1].cpu().numpy(), (ema[1] * np.float32(decay)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------
# hash field
# ---------------------------------------------------------------------------------------------------
K_F, G_F, CONE_F, DT_MIN_F, DT_MAX_F, K_MAX_F = 2, 32, 0.01, 0.002, 0.02, 400  # (steps of 0.6 to 1.6 level-0 cell edges: both levels are used)


@functools.lru_cache(None)
def field_fixture():
    """The field of tests/test_gpu_zzzzzpacked.py (its weights, table scale and box; sdf_bias so that a surface exists) on the OUTERMOST box of
    a K = 2 cascade whose base box is half of it, a ball of set bits per level, and 257 rays from outside the box through it."""
    from lab4d_amd import hashfield
    cfg = {"L": 16, "F": 2, "log2_T": 14, "n_min": 16, "n_max": 512}
    P, cfg = hashfield.make_weights(3, cfg, sdf_bias=0.01)
    P["hash.table"] = P["hash.table"] * 3e3
    base = (P["aabb"] / 2).numpy()
    aabbs = CC.cascade_boxes(K_F, base)
    assert np.array_equal(aabbs[K_F - 1], P["aabb"].numpy().reshape(6))
    occ = CC.cascade_occupancy(K_F, G_F, 0, "ball")
    o, d, tr = PC.outside_rays(257, 21, aabb=P["aabb"].numpy())
    tr[:, 0], tr[:, 1] = 0.0, 3.0
    names = [k for k in P if k != "aabb"]
    g = torch.Generator().manual_seed(7)
    R = o.shape[0]
    cw = [torch.randn(R, 3, generator=g).to(DEV), torch.randn(R, 1, generator=g).to(DEV), torch.randn(R, 1, generator=g).to(DEV)]
    twin = CC.host_march(CC.build_host(), o, d, tr, aabbs, CC.pack_levels(occ), G_F, CONE_F, DT_MIN_F, DT_MAX_F, K_MAX_F)
    return {"cfg": cfg, "P": P, "base": base, "aabbs": aabbs, "occ": occ, "o": o, "d": d, "tr": tr, "names": names, "cw": cw, "R": R, "twin": twin,
            "total": twin["total"], "cap": int(1.5 * twin["total"])}


def params(fx):
    return {k: (v.to(DEV).clone().requires_grad_(True) if k in fx["names"] else v.to(DEV)) for k, v in fx["P"].items()}


def loss_of(fx, rgb, mask, depth):
    return (rgb * fx["cw"][0]).sum() + (mask * fx["cw"][1]).sum() + (depth * fx["cw"][2]).sum()


def march_fixture(fx, casc=None):
    casc = casc or new_cascade(K_F, G_F, fx["occ"], base=fx["base"])
    return casc, packed.march_cone(casc, dev(fx["o"]), dev(fx["d"]), dev(fx["tr"]), CONE_F, DT_MIN_F, DT_MAX_F, fx["cap"], k_max=K_MAX_F)


def test_render_packed_cone_equals_torch_on_the_emitted_rows():
    """fp32, K = 2, G = 32, 257 rays.  Reference: the emitted rows through hashfield.forward, padded per ray to a dense (R, max count) block with
    zero density behind each ray's count, render_utils.compute_weights and a plain weighted sum.  rgb / mask / depth to 1e-4 (the project's
    fp32 bar), the gradients of the table, every Linear and logibeta to 1e-5 relative L2 (the bound of tests/test_gpu_zzzzzpacked.py for the
    same comparison); with_distortion=True against the float64 definition with mid = t and width = steps, to the bar of the distortion tests."""
    from lab4d_amd import hashfield, mlp
    from lab4d_amd import render_utils as RU
    fx = field_fixture()
    casc, rays = march_fixture(fx)
    o, d, tr = dev(fx["o"]), dev(fx["d"]), dev(fx["tr"])
    R, cap = fx["R"], fx["cap"]
    assert 2000 < fx["total"] < cap and len(np.unique(fx["twin"]["level"])) == K_F and len(np.unique(fx["twin"]["steps"])) > 10
    Pp = params(fx)
    rgb, mask, depth, total, ovf, dist = hashfield.render_packed_cone(Pp, fx["cfg"], casc, o, d, tr, CONE_F, DT_MIN_F, DT_MAX_F, cap, prec=mlp.PREC_F32,
                                                                      k_max=K_MAX_F, with_distortion=True)
    assert tuple(rgb.shape) == (R, 3) and tuple(mask.shape) == (R, 1) and tuple(depth.shape) == (R, 1) and tuple(dist.shape) == (R, 1)
    assert int(total) == fx["total"] and not bool(ovf)
    gp = dict(zip(fx["names"], torch.autograd.grad(loss_of(fx, rgb, mask, depth), [Pp[k] for k in fx["names"]])))
    # torch on the same rows
    Pd = params(fx)
    rgb_s, dens_s = hashfield.forward(Pd, fx["cfg"], rays.xyz, rays.dirs, spf=cap, prec=mlp.PREC_F32)
    count, start = rays.ray_count.long(), rays.ray_start.long()
    D = int(count.max())
    j = torch.arange(D, device=DEV)[None, :]
    valid = j < count[:, None]
    idx = torch.where(valid, start[:, None] + j, torch.zeros_like(j))
    dens_d = torch.where(valid, dens_s[idx, 0], torch.zeros((), device=DEV))
    w, _ = RU.compute_weights(dens_d.reshape(1, R, D, 1), rays.deltas[idx].reshape(1, R, D, 1))
    w = w.reshape(R, D)
    mask_d = w.sum(-1, keepdim=True)
    wn = w / (mask_d + 1e-6)
    rgb_d = (wn[:, :, None] * rgb_s[idx]).sum(1)
    depth_d = (wn * rays.t[idx]).sum(1, keepdim=True)
    gd = dict(zip(fx["names"], torch.autograd.grad(loss_of(fx, rgb_d, mask_d, depth_d), [Pd[k] for k in fx["names"]])))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))
    errs = {"rgb": rel(rgb.detach(), rgb_d.detach()), "mask": rel(mask.detach(), mask_d.detach()), "depth": rel(depth.detach(), depth_d.detach())}
    gerrs = {k: float((gp[k] - gd[k]).norm() / gd[k].norm().clamp_min(1e-20)) for k in fx["names"]}
    print("render_packed_cone against torch on the emitted rows:", errs, gerrs)
    assert float(mask_d.detach().max()) > 0.1 and int((count == 0).sum()) > 5  # opaque rays and rays that miss the ball
    for k, e in errs.items():
        assert e < PC.FP32_BAR, (k, e)
    for k, e in gerrs.items():
        assert e < GRAD_BOUND, (k, e)
    for x in (rgb, mask, depth, dist):
        assert float(x.detach()[count == 0].abs().max()) == 0.0
    # the distortion: the float64 definition on the rows' own fp32 density, mid = t, width = steps
    n = min(fx["total"], cap)
    case = {"R": R, "P": cap, "start": rays.ray_start.cpu().numpy(), "count": rays.ray_count.cpu().numpy(), "density": dens_s.detach()[:, 0].cpu().numpy(),
            "deltas": rays.deltas.cpu().numpy(), "mid": rays.t.cpu().numpy(), "width": rays.steps.cpu().numpy(), "g_loss": np.ones(R, np.float32)}
    assert (case["width"][:n] > 0).all()
    ref = DC.ref_distortion(case)
    e = DC.rel_max(dist.detach()[:, 0].cpu().numpy(), ref["loss"])
    print("distortion with width = steps: rel_max %.2e, max %.3e" % (e, ref["loss"].max()))
    assert ref["loss"].max() > 0 and e < DC.FP32_BAR, e
    # without the flags: the five outputs of render_packed, the same values
    five = hashfield.render_packed_cone({k: v.detach() for k, v in Pp.items()}, fx["cfg"], casc, o, d, tr, CONE_F, DT_MIN_F, DT_MAX_F, cap, k_max=K_MAX_F)
    assert len(five) == 5 and torch.equal(five[0], rgb.detach()) and torch.equal(five[2], depth.detach())


def test_update_occupancy_cascade_on_the_field():
    from lab4d_amd import hashfield
    fx = field_fixture()
    Pl = {k: v.to(DEV) for k, v in fx["P"].items()}
    with torch.no_grad():
        probe = occgrid.OccupancyCascade(dev(fx["base"]), K=K_F, G=G_F)
        pts = probe.cell_centers().reshape(-1, 3)
        dirs = torch.zeros_like(pts)
        dirs[:, 2] = 1.0
        dens = hashfield.forward(Pl, fx["cfg"], pts, dirs, spf=pts.shape[0])[1][:, 0].reshape(K_F, -1)
    thresh = float(dens[0].median())
    casc = occgrid.OccupancyCascade(dev(fx["base"]), K=K_F, G=G_F, thresh=thresh)
    assert hashfield.update_occupancy_cascade(Pl, fx["cfg"], casc, chunk=40000) is casc  # (two pieces: G^3 = 32768 per level)
    ema = CC.np_cascade_new(K_F, G_F)
    want = CC.np_cascade_update(ema, dens.cpu().numpy(), K_F, G_F, casc.decay, thresh)
    got = np.stack([OC.unpack(w, G_F) for w in casc.bits.cpu().numpy().view(np.uint32)])
    assert np.array_equal(got, want) and CC.parents_hold(got) and 0 < got[0].sum() < G_F ** 3
    assert casc.n_occupied.tolist() == [int(w.sum()) for w in want]
    with pytest.raises(RuntimeError, match="outermost box"):
        hashfield.update_occupancy_cascade(dict(Pl, aabb=dev(fx["base"])), fx["cfg"], casc)


def sorted_per_ray(lst):
    """a list's own invariants: rows in ray order, t non-decreasing within a ray, the counts clamped to the rows there are"""
    t, start, count = lst.t.cpu().numpy(), lst.ray_start.cpu().numpy(), lst.ray_count.cpu().numpy()
    n = min(int(lst.total), lst.cap)
    assert int(count.sum()) == n and bool(lst.overflow) == (int(lst.total) > lst.cap)
    if not bool(lst.overflow):
        assert np.array_equal(start, np.cumsum(count) - count)
    assert (count >= 0).all() and (start + count <= lst.cap)[count > 0].all()
    r = np.repeat(np.arange(len(count)), count)
    assert np.array_equal(lst.ray_idx.cpu().numpy()[:n], r)
    assert (np.diff(t[:n])[r[1:] == r[:-1]] >= 0).all()
    return n, count


def test_prune_accepts_a_cone_marched_list():
    from lab4d_amd import hashfield
    fx = field_fixture()
    casc, rays = march_fixture(fx)
    Pl = {k: v.to(DEV) for k, v in fx["P"].items()}
    with torch.no_grad():
        dens = hashfield.density(Pl, fx["cfg"], rays.xyz) * 200.0  # (the fixture's field is thin: made opaque, so that rays do end early)
    kept = packed.prune(rays, dens, early_stop_eps=1e-2, alpha_thre=1e-3, aabb=casc.aabbs[K_F - 1])
    n, count = sorted_per_ray(kept)
    assert 0 < n < fx["total"] and (count <= rays.ray_count.cpu().numpy()).all() and not bool(kept.overflow)
    src = kept.src_row.cpu().numpy()[:n]
    assert np.array_equal(kept.t.cpu().numpy()[:n], rays.t.cpu().numpy()[src]) and np.array_equal(kept.deltas.cpu().numpy()[:n], rays.deltas.cpu().numpy()[src])
    cut = packed.prune(rays, dens, early_stop_eps=1e-2, alpha_thre=1e-3, cap=n - 3, aabb=casc.aabbs[K_F - 1])
    assert sorted_per_ray(cut)[0] == n - 3 and bool(cut.overflow)


def test_resample_accepts_a_cone_marched_list():
    from lab4d_amd import hashfield
    fx = field_fixture()
    casc, rays = march_fixture(fx)
    Pl = {k: v.to(DEV) for k, v in fx["P"].items()}
    with torch.no_grad():
        w = packed.weights(hashfield.density(Pl, fx["cfg"], rays.xyz), rays.deltas, rays)
    n_imp = 8
    fine = packed.resample(rays, w, dev(fx["o"]), dev(fx["d"]), n_imp, aabb=casc.aabbs[K_F - 1])
    n, count = sorted_per_ray(fine)
    has_rows = rays.ray_count.cpu().numpy() > 0
    assert np.array_equal(count, np.where(has_rows, n_imp, 0)) and n == n_imp * int(has_rows.sum()) and not bool(fine.overflow)
    # every new row lies inside its source row's interval, and is no wider than it
    src = fine.src_row.cpu().numpy()[:n]
    ln = np.linalg.norm(fx["d"].astype(np.float64), axis=1)[fine.ray_idx.cpu().numpy()[:n]]
    half = rays.deltas.cpu().numpy()[src] / ln / 2
    assert (np.abs(fine.t.cpu().numpy()[:n] - rays.t.cpu().numpy()[src]) <= half + 1e-6).all()  # (t <= 3: four fp32 spacings of slack at the edge)
    assert (fine.deltas.cpu().numpy()[:n] <= rays.deltas.cpu().numpy()[src] * (1 + 1e-6)).all()


def test_merge_accepts_a_cone_marched_list_and_a_uniform_one():
    fx = field_fixture()
    casc, rays = march_fixture(fx)
    uniform = packed.march(casc.level_grid(K_F - 1), dev(fx["o"]), dev(fx["d"]), dev(fx["tr"]), DT_MIN_F, fx["R"] * K_MAX_F, k_max=K_MAX_F)
    assert 0 < int(uniform.total) <= uniform.cap
    merged = packed.merge(rays, uniform)
    n, count = sorted_per_ray(merged)
    assert n == fx["total"] + int(uniform.total) and np.array_equal(count, (rays.ray_count + uniform.ray_count).cpu().numpy()) and not bool(merged.overflow)
    both = torch.cat([rays.t, uniform.t]).cpu().numpy()
    assert np.array_equal(merged.t.cpu().numpy()[:n], both[merged.src.cpu().numpy()[:n]])  # every value is a copy
    steps = packed.merge_rows(merged, rays.steps, torch.full_like(uniform.t, DT_MIN_F))  # per-row values follow, the cone list's steps among them
    assert float(steps[:n].min()) >= np.float32(DT_MIN_F) and float(steps[:n].max()) <= np.float32(DT_MAX_F)
    cut = packed.merge(rays, uniform, cap=n - 5)
    assert sorted_per_ray(cut)[0] == n - 5 and bool(cut.overflow)


def test_march_cone_is_capturable_and_reads_the_bits_at_replay():
    fx = field_fixture()
    lib = CC.build_host()
    casc = new_cascade(K_F, G_F, fx["occ"], base=fx["base"])
    o, d, tr = dev(fx["o"]), dev(fx["d"]), dev(fx["tr"])
    pts = dev(fx["twin"]["xyz"][:1000])
    keys = CC.FIELDS + ("ray_idx", "level", "ray_start", "ray_count", "total", "overflow")

    def run():
        rays = packed.march_cone(casc, o, d, tr, CONE_F, DT_MIN_F, DT_MAX_F, fx["cap"], k_max=K_MAX_F)
        return rays, casc.mask(pts)

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        rays, (mask, level) = run()
    for occ in (fx["occ"], CC.cascade_occupancy(K_F, G_F, 0, "random"), CC.cascade_occupancy(K_F, G_F, 0, "empty"), fx["occ"]):
        casc.bits.copy_(dev(CC.pack_levels(occ).view(np.int32)))
        for k in keys:
            getattr(rays, k).zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = CC.host_march(lib, fx["o"], fx["d"], fx["tr"], fx["aabbs"], CC.pack_levels(occ), G_F, CONE_F, DT_MIN_F, DT_MAX_F, K_MAX_F, cap=fx["cap"])
        CC.assert_same(as_dict(rays), want, "replay")
        want_mask, want_level = CC.host_cascade_mask(lib, fx["twin"]["xyz"][:1000], None, fx["aabbs"], CC.pack_levels(occ), G_F)
        assert np.array_equal(mask.cpu().numpy(), want_mask) and np.array_equal(level.cpu().numpy(), want_level)
    assert int(rays.total) == fx["total"]
