"""Importance resampling of a packed list on the device (csrc/presample.hip through lab4d_amd/packed.py and hashfield.render_packed_resampled):
both resample kernels against the CPU twin (tests/host_harness/presample/presample_host.cpp) WORD FOR WORD, the weights kernel against float64
and against packed.composite's mask, then the host layer -- resample followed by packed.merge with the coarse list,
render_packed_resampled, graph capture."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occgrid_checks as OC  # noqa: E402
import packed_checks as PC  # noqa: E402
import presample_checks as PS  # noqa: E402

from lab4d_amd import _lib, hashfield, mlp, occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIST_KEYS = ("weights", "t", "deltas", "start", "count", "origin", "dir", "aabb")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_resample(case, d, n_imp, u=None, eps=PS.EPS, cap=None, pad=PS.PAD):
    """the library's two calls around torch's exclusive sum on buffers pre-filled with the sentinels of PS.empty_buffers (cap + pad rows: the
    rows behind the capacity show that they were left alone; cdf likewise in the rows of no ray) -> the dict of PS.host_resample"""
    R, P = case["R"], case["P"]
    cdf, mass = torch.full((P,), float(PS.SENTINEL_F), device=DEV), torch.full((R,), float(PS.SENTINEL_F), device=DEV)
    count = torch.full((R,), int(PS.SENTINEL_I), dtype=torch.int32, device=DEV)
    _lib.call("packed_resample_count", d["weights"], d["start"], d["count"], R, P, n_imp, eps, cdf, mass, count)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count
    if cap is None:
        cap = int(count.sum())
    out = {k: dev(v) for k, v in PS.empty_buffers(case, cap, pad).items()}
    _lib.call("packed_resample_write", d["weights"], cdf, mass, d["t"], d["deltas"], d["start"], d["count"], start, R, P, d["origin"], d["dir"],
              None if u is None else dev(u), n_imp, eps, cap, d["aabb"], out["t"], out["deltas"], out["xyz"], out["dirs"], out["ray_idx"], out["src_row"],
              out["ray_count"], out["total"], out["overflow"])
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(ray_start=start.cpu().numpy(), count=count.cpu().numpy(), cdf=cdf.cpu().numpy(), mass=mass.cpu().numpy(), total=int(res["total"][0]),
               overflow=bool(res["overflow"][0]), R=R, cap=cap)
    return res


@pytest.mark.parametrize("R", PS.RAYS)
def test_kernels_equal_the_cpu_twin_word_for_word(R):
    """the lists of tests/presample_checks.py (lengths 0 / 1 / 2 / 63 / 64 / 65 / 129 / 200, gaps, a (start, count) that leaves [0, P),
    weights with zeros, a NaN and a negative value, an all-zero ray) at n_imp = 1 / 2 / 64 / 65 / 130, with the stratified queries, with a
    caller's sorted u and with a caller's u that is unsorted, partly outside [0, 1] and holds NaN, at the capacities total, total - 1, the middle of a ray and 0: every output array of both kernels, total and overflow;
    the sentinels show what was left alone"""
    lib = PS.build_host()
    case = PS.make_list(R, seed=500 + R)
    d = {k: dev(case[k]) for k in LIST_KEYS}
    for n_imp in PS.N_IMP:
        for u in (None, PS.uniforms(case, n_imp, seed=n_imp), PS.unsorted_uniforms(case, n_imp, seed=n_imp)):
            full = PS.host_resample(lib, case, n_imp, u)
            for cap in PS.capacities(full):
                ref, got = PS.host_resample(lib, case, n_imp, u, cap=cap), device_resample(case, d, n_imp, u, cap=cap)
                PS.assert_same(got, ref, (R, n_imp, u is not None, cap))
                assert (got["src_row"][cap:] == PS.SENTINEL_I).all() and (got["t"][cap:] == PS.SENTINEL_F).all() and (got["xyz"][cap:] == PS.SENTINEL_F).all()
    got = device_resample(case, d, 65, eps=0.0)
    PS.assert_same(got, PS.host_resample(lib, case, 65, eps=0.0), (R, "eps = 0"))
    assert R < 3 or (got["count"][R - 3] == 0 and got["mass"][R - 3] == 0)  # the all-zero ray


@pytest.mark.parametrize("R", [65, 1025])
def test_order_rule_decides_t_for_an_unsorted_u(R):
    """the ORDER rule on the device: a caller's u that is unsorted, partly outside [0, 1] and holds NaN, at n_imp = 65 and 130 so that the
    carry of the running maximum crosses the 64-sample chunks.  The kernel's t equals the twin's word for word, it is non-decreasing
    within every ray, it is NOT the placed depths (numpy's t' of the PLACE rule: most words differ, so a write kernel without the max scan
    fails here), and behind the first chunk rows hold a maximum reached in an earlier chunk (a kernel without the carry fails here).  The
    list then merges with its source list into a list that is non-decreasing in t: the precondition the rule exists for."""
    lib = PS.build_host()
    case = PS.make_list(R, seed=500 + R)
    d = {k: dev(case[k]) for k in LIST_KEYS}
    for n_imp in (65, 130):
        u = PS.unsorted_uniforms(case, n_imp, seed=n_imp)
        ref, got = PS.host_resample(lib, case, n_imp, u), device_resample(case, d, n_imp, u)
        PS.assert_same(got, ref, (R, n_imp, "unsorted u"))
        total = got["total"]
        placed, t = PS.ref_resample(case, n_imp, u)["t_placed"].reshape(-1, n_imp), got["t"][:total].reshape(-1, n_imp)
        assert total == placed.size > 0 and (np.diff(t, axis=1) >= 0).all() and np.array_equal(t, np.maximum.accumulate(placed, axis=1))
        assert (np.diff(placed, axis=1) < 0).any(axis=1).mean() > 0.9 and (t != placed).mean() > 0.5
        for c0 in range(64, n_imp, 64):
            carried = (t[:, c0:] == t[:, c0 - 1:c0]) & (placed[:, c0:] < t[:, c0:])
            assert carried.any(axis=1).mean() > 0.5, (n_imp, c0)
    src = types.SimpleNamespace(t=d["t"], deltas=d["deltas"], ray_start=d["start"], ray_count=d["count"])
    fine = packed.resample(src, d["weights"], d["origin"], d["dir"], 130, aabb=d["aabb"], u=dev(u))
    assert int(fine.total) == total and torch.equal(fine.t[:total].cpu(), torch.from_numpy(got["t"][:total]))
    m = packed.merge(src, fine)
    n = int(m.total)
    mt, idx = m.t[:n].cpu().numpy(), m.ray_idx[:n].cpu().numpy()
    assert n == int(fine.total) + sum(PS.rows_of(case, r)[1] for r in range(R)) and (np.diff(idx) >= 0).all() and (np.diff(mt)[np.diff(idx) == 0] >= 0).all()


def test_every_wave_runs_several_rays():
    """66,000 short rays: more than the 4 x 16,384 rays that one pass of the largest grid takes, so the first blocks' waves come round again"""
    lib = PS.build_host()
    rng = np.random.default_rng(8)
    R, n_imp = 66000, 3
    count = rng.choice(np.int32([0, 1, 2, 3, 70]), R, p=[0.3, 0.3, 0.2, 0.19, 0.01])
    P = int(count.sum())
    start = (np.cumsum(count) - count).astype(np.int32)
    t = np.zeros(P, np.float32)
    for s, n in zip(start, count):
        t[s:s + n] = np.arange(1, n + 1) / 64.0
    d = rng.standard_normal((R, 3)).astype(np.float32)
    case = {"R": R, "P": P, "start": start, "count": count, "aabb": PS.AABB, "origin": rng.standard_normal((R, 3)).astype(np.float32), "dir": d, "t": t,
            "deltas": np.repeat(PS.dir_length(d) / np.float32(64.0), count).astype(np.float32), "weights": rng.random(P).astype(np.float32)}
    ref = PS.host_resample(lib, case, n_imp)
    got = device_resample(case, {k: dev(case[k]) for k in LIST_KEYS}, n_imp, cap=ref["cap"])
    assert ref["total"] == n_imp * int((count > 0).sum()) > 100000
    PS.assert_same(got, ref, "66000 rays")


def test_weights_against_float64_and_the_composite_mask():
    """lab4d_packed_weights against the float64 compute_weights per ray at the 1e-4 bar (absolute: a weight lies in [0, 1]); its per-ray
    sum against packed.composite's mask at the same bar; a NaN and a negative density count as tau = 0; the rows of no ray are zero"""
    case = PS.make_list(65, seed=3)
    rng = np.random.default_rng(4)
    P, R = case["P"], 65
    density = (rng.random(P) * 40).astype(np.float32)
    rays = types.SimpleNamespace(ray_start=dev(case["start"]), ray_count=dev(case["count"]))
    _, mask = packed.composite(dev(density), dev(case["deltas"]), {"one": torch.ones(P, 1, device=DEV)}, rays)
    s3, _ = PS.rows_of(case, 3)
    bad = density.copy()
    bad[s3 + 1], bad[s3 + 2] = np.nan, -3.0
    for dens in (density, bad):
        w, trans = packed.weights(dev(dens)[:, None], dev(case["deltas"]), rays, with_trans=True)
        assert tuple(w.shape) == (P,) and tuple(trans.shape) == (R,) and w.dtype == trans.dtype == torch.float32
        w, trans = w.cpu().numpy(), trans.cpu().numpy()
        owned, sums, errs = np.zeros(P, bool), np.zeros(R), {"w": 0.0, "trans": 0.0}
        for r in range(R):
            s, n = PS.rows_of(case, r)
            owned[s:s + n] = True
            with np.errstate(invalid="ignore"):
                tau = dens[s:s + n].astype(np.float64) * case["deltas"][s:s + n].astype(np.float64)
            tau = np.where(tau > 0, tau, 0.0)
            want = (1 - np.exp(-tau)) * np.exp(-(np.cumsum(tau) - tau))
            sums[r] = w[s:s + n].astype(np.float64).sum()
            errs["w"] = max(errs["w"], float(np.abs(w[s:s + n] - want).max(initial=0)))
            errs["trans"] = max(errs["trans"], abs(float(trans[r]) - float(np.exp(-tau.sum()))))
        print("packed.weights:", {k: "%.2e" % v for k, v in errs.items()})
        assert errs["w"] <= 1e-4 and errs["trans"] <= 1e-4 and (w[~owned] == 0).all() and np.isfinite(w).all() and trans[-2] == 1
        if dens is density:
            err = float(np.abs(sums - mask[:, 0].cpu().numpy().astype(np.float64)).max())
            print("sum of weights against the composite's mask: %.2e" % err)
            assert err <= 1e-4 and sums.max() > 0.9
    assert w[s3 + 1] == 0 and w[s3 + 2] == 0
    assert np.array_equal(packed.weights(dev(bad), dev(case["deltas"]), rays).cpu().numpy(), w)  # without trans: the same weights


# ---------------------------------------------------------------------------------------------------
# a marched list
# ---------------------------------------------------------------------------------------------------
G, K_MAX, DT = 32, 200, 0.015
N_FINE = 24


def new_grid(aabb, occ):
    grid = occgrid.OccupancyGrid(dev(aabb), G=G)
    grid.bits.copy_(dev(OC.pack(occ).view(np.int32)))
    return grid


@functools.lru_cache(None)
def marched_list():
    """65 rays marched through the sphere grid of tests/occgrid_checks.py, with a random density on its rows"""
    o, d, tr = PC.outside_rays(65, 21, aabb=OC.AABB)
    tr[:, 0], tr[:, 1] = 0.0, 3.0
    grid = new_grid(OC.AABB, OC.sphere_occupancy(G))
    total = int(packed.march(grid, dev(o), dev(d), dev(tr), DT, 0, k_max=K_MAX).total)
    rays = packed.march(grid, dev(o), dev(d), dev(tr), DT, total + 9, k_max=K_MAX)
    assert int(rays.total) == total > 100 and int(rays.ray_count.max()) > 5
    dens = (torch.rand(rays.cap, 1, generator=torch.Generator().manual_seed(5)) * 40).to(DEV)
    return rays, total, grid, dev(o), dev(d), dens


def test_resample_then_merge_with_the_coarse_list():
    """packed.resample of a marched list, merged with that list: the result is non-decreasing in t within every ray and contains every row
    of both lists (src is a permutation of them); the resampled list alone is a PrunedRays laid out like a march's"""
    rays, total, grid, o, d, dens = marched_list()
    w = packed.weights(dens, rays.deltas, rays)
    fine = packed.resample(rays, w, o, d, N_FINE, aabb=grid.aabb)
    live = int((rays.ray_count > 0).sum())
    assert isinstance(fine, packed.PrunedRays) and fine.cap == 65 * N_FINE and fine.R == 65 and fine.overflow.dtype == torch.bool
    assert int(fine.total) == N_FINE * live and not bool(fine.overflow) and 10 < live < 65
    assert torch.equal(fine.ray_count, torch.where(rays.ray_count > 0, N_FINE, 0).to(torch.int32))
    n = int(fine.total)
    src = fine.src_row[:n].long()
    assert torch.equal(rays.ray_idx[src], fine.ray_idx[:n]) and bool((fine.src_row[n:] == -1).all()) and bool((fine.ray_idx[n:] == -1).all())
    assert bool((fine.deltas[:n] <= rays.deltas[src]).all()) and bool((fine.deltas[:n] > 0).all()) and bool((fine.t[n:] == 0).all())
    half = rays.deltas[src] / d.norm(dim=1)[fine.ray_idx[:n].long()] * 0.5000001
    assert bool(((fine.t[:n] - rays.t[src]).abs() <= half).all())  # inside the source row's interval
    assert torch.allclose(fine.xyz[:n], o[fine.ray_idx[:n].long()] + fine.t[:n, None] * d[fine.ray_idx[:n].long()], atol=1e-6)
    m = packed.merge(rays, fine)
    assert int(m.total) == total + n and not bool(m.overflow)
    t, idx = m.t[:total + n].cpu().numpy(), m.ray_idx[:total + n].cpu().numpy()
    assert (np.diff(idx) >= 0).all() and (np.diff(t)[np.diff(idx) == 0] >= 0).all()
    got = np.sort(m.src[:total + n].cpu().numpy())
    assert np.array_equal(got, np.concatenate([np.arange(total), rays.cap + np.arange(n)]))
    # a cap below the total: the list is cut like a march's
    cut = packed.resample(rays, w, o, d, N_FINE, aabb=grid.aabb, cap=n - 5)
    assert int(cut.total) == n and bool(cut.overflow) and int(cut.ray_count.sum()) == n - 5 and torch.equal(cut.t, fine.t[:n - 5])


# ---------------------------------------------------------------------------------------------------
# the hash field, coarse to fine
# ---------------------------------------------------------------------------------------------------
R_FIELD = 256


@functools.lru_cache(None)
def field_fixture():
    """a small hash field (log2_T 12, n_max 128) from make_weights behind the sphere grid; 256 rays aimed at its box"""
    P, cfg = hashfield.make_weights(3, {"L": 16, "F": 2, "log2_T": 12, "n_min": 16, "n_max": 128})
    P["hash.table"] = P["hash.table"] * 1e3
    o, d, tr = PC.outside_rays(R_FIELD, 21, aabb=P["aabb"].numpy())
    tr[:, 0], tr[:, 1] = 0.0, 3.0
    occ = OC.sphere_occupancy(G)
    cap = int(packed.march(new_grid(P["aabb"].numpy(), occ), dev(o), dev(d), dev(tr), DT, 0, k_max=K_MAX).total) + 64
    assert cap > 64 + 1000
    return {"P": P, "cfg": cfg, "o": dev(o), "d": dev(d), "tr": dev(tr), "occ": occ, "cap": cap}


def test_render_packed_resampled():
    fx = field_fixture()
    P = {k: v.to(DEV).clone().requires_grad_(k != "aabb") for k, v in fx["P"].items()}
    grid = new_grid(fx["P"]["aabb"].numpy(), fx["occ"])
    out = hashfield.render_packed_resampled(P, fx["cfg"], grid, fx["o"], fx["d"], fx["tr"], DT, fx["cap"], N_FINE, prec=mlp.PREC_F32, k_max=K_MAX)
    rgb, mask, depth, total, ovf, total_fine, ovf_fine = out
    assert tuple(rgb.shape) == (R_FIELD, 3) and tuple(mask.shape) == tuple(depth.shape) == (R_FIELD, 1)
    for k, x in zip(("rgb", "mask", "depth"), (rgb, mask, depth)):
        assert bool(torch.isfinite(x).all()), k
    rays = packed.march(grid, fx["o"], fx["d"], fx["tr"], DT, fx["cap"], k_max=K_MAX)
    live = int((rays.ray_count > 0).sum())
    assert int(total) == int(rays.total) > 1000 and not bool(ovf) and not bool(ovf_fine) and 50 < live < R_FIELD
    assert int(total_fine) == N_FINE * live and float(mask.detach().max()) > 0.05
    assert bool((mask[rays.ray_count == 0] == 0).all()) and bool((rgb[rays.ray_count == 0] == 0).all())
    g = torch.Generator().manual_seed(9)
    w = [torch.randn(R_FIELD, c, generator=g).to(DEV) for c in (3, 1, 1)]
    sum((x * y).sum() for x, y in zip((rgb, mask, depth), w)).backward()
    for k, v in P.items():
        if k != "aabb":
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()), k
    assert float(P["hash.table"].grad.abs().max()) > 0 and float(P["logibeta"].grad.abs().max()) > 0 and float(P["hash.color.4.weight"].grad.abs().max()) > 0
    # a caller's u and a fine capacity below the total
    u = torch.rand(R_FIELD, N_FINE, generator=g).sort(dim=1).values.to(DEV)
    with torch.no_grad():
        cut = hashfield.render_packed_resampled(P, fx["cfg"], grid, fx["o"], fx["d"], fx["tr"], DT, fx["cap"], N_FINE, fine_cap=N_FINE * live - 7, u=u, k_max=K_MAX)
    assert int(cut[5]) == N_FINE * live and bool(cut[6]) and bool(torch.isfinite(cut[0]).all())
    # the grid emptied: nothing is marched, nothing is resampled, everything renders zero
    grid.bits.zero_()
    with torch.no_grad():
        none = hashfield.render_packed_resampled(P, fx["cfg"], grid, fx["o"], fx["d"], fx["tr"], DT, fx["cap"], N_FINE, k_max=K_MAX)
    assert all(bool((x == 0).all()) for x in none[:3]) and int(none[3]) == 0 and int(none[5]) == 0 and not bool(none[4]) and not bool(none[6])


def test_weights_and_resample_are_capturable():
    """weights + resample + composite in one torch.cuda.graph: a linear capture on one stream; the replay gives the eager bits, and again
    after the density changed in place"""
    rays, total, grid, o, d, dens = marched_list()
    dens = dens.clone()
    rgb = torch.rand(65 * N_FINE, 3, generator=torch.Generator().manual_seed(1)).to(DEV)

    def run():
        with torch.no_grad():
            fine = packed.resample(rays, packed.weights(dens, rays.deltas, rays), o, d, N_FINE, aabb=grid.aabb)
            rendered, mask = packed.composite(fine.deltas * 30.0, fine.deltas, {"rgb": rgb, "depth": fine.t[:, None]}, fine)
            return fine.t, fine.deltas, fine.xyz, fine.src_row, fine.ray_count, fine.total, rendered["rgb"], rendered["depth"], mask

    side = torch.cuda.Stream()  # the warm-up runs on a side stream; the capture itself is linear
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager0 = [x.clone() for x in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for x in outs:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(outs, eager0):
        assert torch.equal(x, y)
    with torch.no_grad():  # the mass moves to the far end of every ray
        dens.mul_(torch.linspace(1e-4, 1.0, dens.shape[0], device=DEV)[:, None] ** 4)
    graph.replay()
    torch.cuda.synchronize()
    eager1 = [x.clone() for x in run()]
    for x, y in zip(outs, eager1):
        assert torch.equal(x, y)
    assert not torch.equal(eager1[0], eager0[0]) and not torch.equal(eager1[7], eager0[7])  # t, depth: it did change
