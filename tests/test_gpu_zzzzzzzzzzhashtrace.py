"""Sphere tracing of the hash field's SDF on the device (csrc/hashtrace.hip through lab4d_amd/hashtrace.py and hashfield.trace_surface /
render_surface): the kernel against its CPU twin (tests/hashtrace_checks.py; the hashsdf forward is not bit-equal to its twin, so neither is this
kernel: statuses equal, t_hit within 5 eps / len, nothing word for word), the invariants through the float64 oracle, the degenerate rays,
trace_surface behind an occupancy grid, render_surface against the float64 root and normal, its implicit-surface gradient, graph capture
and the argument checks."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashtrace_checks as TC  # noqa: E402
from test_hashtrace_host import N_HIT, N_MISS, check_hits, check_invariants  # noqa: E402

from lab4d_amd import hashfield, hashtrace, occgrid  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 63, 64, 65, 1025)
NEAR = 1e-4  # a hit point with x01 * res_0 within this of an integer is left out of the normal comparison: fp32 and float64 may pick different cells


def on_device(P):
    return {k: v.to(DEV) for k, v in P.items()}


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def device_trace(P, cfg, o, d, tr, **kw):
    Pd = on_device(P)
    out = hashtrace.trace(*dev(o, d, tr), Pd["aabb"], Pd["hash.table"], hashfield.resolutions(cfg, DEV), cfg["log2_T"], Pd["hash.geo.0.weight"],
                          Pd["hash.geo.0.bias"], Pd["hash.geo.2.weight"][0], Pd["hash.geo.2.bias"][:1], **dict(TC.DEFAULTS, **kw))
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(None)
def mixed_rays(name):
    """1,025 rays of an analytic field, hit and miss rays interleaved two to one (shared, never modified); the first 192 are the sets of the CPU suite"""
    n = max(SIZES)
    sets = [TC.rays(name, "hit", N_HIT), TC.rays(name, "miss", N_MISS), TC.rays(name, "hit", n, seed=1), TC.rays(name, "miss", n // 2, seed=1)]
    o, d, tr = (np.concatenate([s[i] for s in sets[:2]]) for i in range(3))
    order = np.argsort(np.concatenate([np.arange(n) * 1.0, np.arange(n // 2) * 2.0 + 0.5]), kind="stable")
    more = [np.concatenate([s[i] for s in sets[2:]])[order] for i in range(3)]
    return tuple(np.ascontiguousarray(np.concatenate([a, b])[:n]) for a, b in zip((o, d, tr), more))


@pytest.mark.parametrize("name", ["sphere", "two", "sphere4"])
def test_kernel_against_the_twin_on_hit_and_miss_rays(name):
    host = TC.build_host()
    P, cfg = TC.field(name)
    o, d, tr = mixed_rays(name)
    ref = TC.host_trace(host, P, cfg, o, d, tr)
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    assert (ref[1] == TC.MISS).sum() > 300 and np.isin(ref[1], (TC.CONVERGED, TC.BRACKETED)).sum() > 600
    for R in SIZES:
        t_hit, status, n_eval, sdf_hit = device_trace(P, cfg, o[:R], d[:R], tr[:R])
        assert np.array_equal(status, ref[1][:R]), (R, np.nonzero(status != ref[1][:R])[0][:8])
        err = np.abs(t_hit.astype(np.float64) - ref[0][:R]) * ln[:R] / TC.EPS
        print("%s R = %d: max |t_hit - twin| * len = %.3f eps, n_eval equal on %d of %d" % (name, R, err.max(), (n_eval == ref[2][:R]).sum(), R))
        assert err.max() <= TC.T_BOUND, (R, err.max())
        assert (n_eval <= 128 + 8).all() and np.abs(sdf_hit - ref[3][:R]).max() <= 2 * TC.EPS
    # and the device's own hits against the float64 root, on the sets of the CPU suite
    t_hit, status, _, _ = device_trace(P, cfg, o[:N_HIT], d[:N_HIT], tr[:N_HIT])
    check_hits(name, t_hit, status, d[:N_HIT])
    t_hit, status, _, _ = device_trace(P, cfg, o[N_HIT:N_HIT + N_MISS], d[N_HIT:N_HIT + N_MISS], tr[N_HIT:N_HIT + N_MISS])
    t_clip, _ = TC.host_clip(host, o[N_HIT:N_HIT + N_MISS], d[N_HIT:N_HIT + N_MISS], tr[N_HIT:N_HIT + N_MISS], P)
    assert (status == TC.MISS).all() and np.array_equal(t_hit, t_clip[:, 1])  # (the clip is plain rounded arithmetic: word for word)


@pytest.mark.parametrize("name", ["sphere", "random"])
def test_invariants_through_the_float64_oracle(name):
    host = TC.build_host()
    P, cfg = TC.field(name)
    o, d, tr = TC.rays(name, "generic", 1025)
    for R in SIZES:
        clip = TC.host_clip(host, o[:R], d[:R], tr[:R], P)
        check_invariants(P, cfg, o[:R], d[:R], tr[:R], clip, *device_trace(P, cfg, o[:R], d[:R], tr[:R]), need_hits=name == "random" and R > 1000)
    kw = dict(step_scale=0.5, min_step=0.002, max_steps=9, n_bisect=32)
    check_invariants(P, cfg, o, d, tr, TC.host_clip(host, o, d, tr, P), *device_trace(P, cfg, o, d, tr, **kw), **kw)


def test_degenerate_rays_on_the_device():
    host = TC.build_host()
    P, cfg = TC.field("sphere")
    o, d, tr, _ = TC.degenerate_rays()
    for kw in (dict(), dict(max_steps=1024, n_bisect=0)):
        got = device_trace(P, cfg, o, d, tr, **kw)
        TC.check_degenerate(*got, **{k: v for k, v in dict(TC.DEFAULTS, **kw).items() if k in ("max_steps", "n_bisect")})
        assert np.array_equal(got[1], TC.host_trace(host, P, cfg, o, d, tr, **kw)[1])
    out = device_trace(P, cfg, o[:0], d[:0], tr[:0])  # R = 0
    assert all(a.size == 0 for a in out)


def test_trace_surface_behind_an_occupancy_grid():
    P, cfg = TC.field("sphere")
    Pd = on_device(P)
    o, d, tr = (np.concatenate([TC.rays("sphere", "hit", N_HIT)[i], TC.rays("sphere", "miss", N_MISS)[i]]) for i in range(3))
    od, dd, trd = dev(o, d, tr)
    grid = occgrid.OccupancyGrid(Pd["aabb"], G=32)
    half_diag = 0.5 * float(torch.linalg.vector_norm((Pd["aabb"][1] - Pd["aabb"][0]) / 32))
    grid.update((grid.cell_centers().norm(dim=-1) <= 0.08 + half_diag).float())  # every cell that holds a point of the ball
    plain = hashfield.trace_surface(Pd, cfg, od, dd, trd)
    behind = hashfield.trace_surface(Pd, cfg, od, dd, trd, grid=grid)
    _, seen = grid.ray_span(od, dd, trd)
    seen = seen.cpu().numpy()
    assert seen[:N_HIT].all() and 0 < (~seen).sum() < N_MISS + 1
    st, t = behind.status.cpu().numpy(), behind.t.cpu().numpy()
    assert (st[~seen] == TC.MISS).all() and np.array_equal(t[~seen], tr[~seen, 0]) and (behind.n_eval.cpu().numpy()[~seen] == 0).all()
    assert np.array_equal(st[:N_HIT], plain.status.cpu().numpy()[:N_HIT]) and behind.hit.cpu().numpy()[:N_HIT].all() and not behind.hit.cpu().numpy()[N_HIT:].any()
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    err = np.abs(t[:N_HIT].astype(np.float64) - plain.t.cpu().numpy()[:N_HIT]) * ln[:N_HIT] / TC.EPS
    print("hit rays behind the grid: max difference %.3f eps; n_eval %.2f -> %.2f" % (err.max(), plain.n_eval[:N_HIT].float().mean(), behind.n_eval[:N_HIT].float().mean()))
    assert err.max() <= TC.T_BOUND
    check_hits("sphere", t[:N_HIT], st[:N_HIT], d[:N_HIT])
    assert torch.equal(behind.xyz, od + behind.t[:, None] * dd) and behind.sdf.shape == (N_HIT + N_MISS,)


def test_render_surface():
    P, cfg = TC.field("sphere")
    Pd = on_device(P)
    o, d, tr = (np.concatenate([TC.rays("sphere", "hit", N_HIT)[i], TC.rays("sphere", "miss", N_MISS)[i]]) for i in range(3))
    od, dd, trd = dev(o, d, tr)
    with torch.no_grad():
        rgb, mask, depth, normal = hashfield.render_surface(Pd, cfg, od, dd, trd)
        s = hashfield.trace_surface(Pd, cfg, od, dd, trd)
    assert rgb.shape == (192, 3) and mask.shape == (192, 1) and depth.shape == (192, 1) and normal.shape == (192, 3)
    assert torch.equal(mask[:, 0].bool(), s.hit) and bool(s.hit[:N_HIT].all()) and not bool(s.hit[N_HIT:].any())
    for out in (rgb, mask, depth, normal):
        assert not out[N_HIT:].any()  # missed rays: exactly zero
    check_hits("sphere", depth[:N_HIT, 0].cpu().numpy(), s.status[:N_HIT].cpu().numpy(), d[:N_HIT])
    assert torch.equal(depth[:N_HIT, 0], s.t[:N_HIT])
    xyz = s.xyz[:N_HIT].cpu()
    _, g64 = TC.sdf64(P, cfg, xyz.double(), with_grad=True)
    n64 = torch.nn.functional.normalize(g64, dim=-1)
    p0 = ((xyz.double() - P["aabb"][0].double()) / (P["aabb"][1].double() - P["aabb"][0].double())) * TC.res_list(cfg)[0]
    left_out = ((p0 - p0.round()).abs() < NEAR).any(-1)
    assert float(left_out.float().mean()) < 0.01
    err = (normal[:N_HIT].cpu().double() - n64).abs().max(-1).values[~left_out]
    print("normal: max difference %.2e (%d of %d left out near a cell face); |grad| %.3f .. %.3f" % (err.max(), left_out.sum(), N_HIT, g64.norm(dim=-1).min(),
                                                                                                     g64.norm(dim=-1).max()))
    assert float(err.max()) <= 1e-3
    unit = torch.nn.functional.normalize(dd[:N_HIT], dim=-1)
    want = hashfield.forward(Pd, cfg, s.xyz[:N_HIT].contiguous(), unit, spf=N_HIT, get_density=False)[0]
    assert float((rgb[:N_HIT] - want).abs().max()) < 1e-5 and float(rgb[:N_HIT].min()) > 0


def test_render_surface_differentiable():
    P, cfg = TC.field("sphere")
    Pd = on_device(P)
    for k in ("hash.table", "hash.geo.0.weight", "hash.geo.0.bias", "hash.geo.2.weight", "hash.geo.2.bias"):
        Pd[k].requires_grad_(True)
    o, d, tr = (np.concatenate([TC.rays("sphere", "hit", N_HIT)[i], TC.rays("sphere", "miss", N_MISS)[i]]) for i in range(3))
    od, dd, trd = dev(o, d, tr)
    with torch.no_grad():
        plain = hashfield.render_surface(Pd, cfg, od, dd, trd)
        s = hashfield.trace_surface(Pd, cfg, od, dd, trd)
        grad = hashfield.sdf_gradient(Pd, cfg, s.xyz.contiguous())[1]
    rgb, mask, depth, normal = hashfield.render_surface(Pd, cfg, od, dd, trd, differentiable=True)
    assert torch.equal(depth, plain[2]) and torch.equal(mask, plain[1]) and depth.requires_grad  # bit for bit
    assert float((rgb.detach() - plain[0]).abs().max()) < 1e-6
    g_bias, g_table = torch.autograd.grad(depth.sum(), [Pd["hash.geo.2.bias"], Pd["hash.table"]], retain_graph=True)
    gd = (grad.double() * dd.double()).sum(-1)[s.hit]
    assert float(gd.abs().min()) > 1e-6
    want = -float((1.0 / gd).sum())
    print("d sum(depth) / d b2: %.6f, -sum 1 / (grad . d): %.6f" % (float(g_bias[0]), want))
    assert abs(float(g_bias[0]) - want) <= 1e-5 * abs(want) and not g_bias[1:].any()
    assert bool(g_table.any()) and bool(torch.isfinite(g_table).all())
    g_color, = torch.autograd.grad(rgb.sum(), [Pd["hash.table"]])  # the colour reaches the table through the point as well
    assert bool(g_color.any())


def test_graph_capture():
    """trace_surface captured in a torch.cuda.graph, the table changed between replays, the replay against eager"""
    P, cfg = TC.field("sphere")
    Pd = on_device(P)
    o, d, tr = TC.rays("sphere", "hit", N_HIT)
    od, dd, trd = dev(o, d, tr)
    res = hashfield.resolutions(cfg, DEV)  # (a host-to-device copy: made before the capture)
    step = lambda: hashfield.trace_surface(Pd, cfg, od, dd, trd, res=res)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager0 = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, eager0))
    with torch.no_grad():
        Pd["hash.table"][0, :, 0] -= 0.01  # the sphere grows by 0.01 between replays
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outs]
    eager1 = step()
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager1))
    ln = torch.linalg.vector_norm(dd, dim=-1)
    assert float(((eager0.t - eager1.t) * ln).min()) > 0.009  # and it did change: every hit comes at least 0.01 earlier


def test_argument_errors_arrive_before_any_launch():
    P, cfg = TC.field("sphere")
    Pd = on_device(P)
    od, dd, trd = dev(*TC.rays("sphere", "hit", N_HIT))
    with pytest.raises(RuntimeError, match=r"max_steps = 2000 outside \[1, 1024\]"):
        hashfield.trace_surface(Pd, cfg, od, dd, trd, max_steps=2000)
    with pytest.raises(RuntimeError, match="disagree"):
        hashfield.trace_surface(Pd, cfg, od, dd[:5], trd)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hashfield.trace_surface(Pd, cfg, od.cpu(), dd, trd)
    from lab4d_amd import _lib
    lib = _lib.lib()
    p = _lib.ptr(od)
    rc = lib.lab4d_hashsdf_trace(p, p, p, p, 4, p, p, 16, 12, 2, p, p, p, p, 1e-4, 1.0, 1e-4, 128, 40, p, p, p, p, _lib.stream())
    assert rc == -1 and "n_bisect = 40" in lib.lab4d_last_error().decode()
    rc = lib.lab4d_hashsdf_trace(p, p, p, p, 4, p, p, 16, 12, 2, p, p, p, p, 1e-4, 1.0, 1e-4, 128, 8, p, None, p, p, _lib.stream())
    assert rc == -1 and "null pointer (t_hit" in lib.lab4d_last_error().decode()
    torch.cuda.synchronize()
