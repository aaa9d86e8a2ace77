"""Ray casting against a triangle mesh on the device (csrc/meshray.hip through lab4d_amd/meshray.py and proxy.ray_range): the kernels against
their CPU twin bit for bit (tests/meshray_checks.py; tests/test_meshray_host.py pins the twin against float64), the cell lists after sorting,
the degenerate rays, a marching-cubes sphere against the analytic one, proxy.ray_range in front of the sphere tracer, the gradient of the hit
point in the vertices, graph capture and the argument checks."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashtrace_checks as TC  # noqa: E402
import mesh_checks as SC  # noqa: E402
import meshray_checks as MC  # noqa: E402
from test_meshray_host import check_against_float64  # noqa: E402

from lab4d_amd import hashfield, mesh, meshray, proxy  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES_F = (0, 1, 255, 256, 257, 1280)
SIZES_G = (1, 2, 5, 32)


def dev(*arrays):
    out = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)
    return out[0] if len(out) == 1 else out


def as_numpy(hits):
    return {k: getattr(hits, k).cpu().numpy() for k in ("t", "face", "u", "v", "front", "n_tests")}


def device_grid(verts, faces, G, aabb=None):
    return meshray.MeshGrid(dev(verts), dev(faces), G=G, aabb=None if aabb is None else dev(np.asarray(aabb, np.float32).reshape(2, 3)))


def test_kernels_against_the_twin():
    """F in {0, 1, 255, 256, 257, 1280} (the first F faces of the icosphere in its box), R in {1, 63, 64, 65, 1025}, G in {1, 2, 5, 32}: the packed
    faces and t, face, u, v, front word for word, n_tests equal, the cell lists equal after sorting"""
    host = MC.build_host()
    verts, faces = MC.icosphere()
    box = MC.default_aabb(verts)
    o, d, tr = MC.mixed_rays("icosphere")
    od, dd, trd = dev(o, d, tr)
    for F in SIZES_F:
        for G in SIZES_G:
            twin = MC.host_build(host, verts, faces[:F], G, aabb=box)
            want = MC.host_cast(host, twin, o, d, tr)
            grid = device_grid(verts, faces[:F], G, aabb=box)
            if F:
                assert np.array_equal(grid.tris.cpu().numpy().view(np.int32).reshape(F, 12), twin["tris"].view(np.int32))
                assert np.array_equal(grid.cell_start.cpu().numpy(), twin["cell_start"]) and grid.cell_list.numel() == twin["cell_list"].size
                assert MC.lists_of(grid.cell_start.cpu().numpy(), grid.cell_list.cpu().numpy()) == MC.lists_of(twin["cell_start"], twin["cell_list"])
            for R in MC.SIZES_R:
                got = as_numpy(grid.cast(od[:R], dd[:R], trd[:R]))
                sl = {k: v[:R] for k, v in want.items()}
                assert MC.same_hits(got, sl), (F, G, R, [int((got[k] != sl[k]).sum()) for k in ("t", "face", "u", "v", "front")])
                assert np.array_equal(got["n_tests"], sl["n_tests"]), (F, G, R)
        if F == 1280:
            assert (want["face"] >= 0).sum() > 600 and (want["face"] < 0).sum() > 300
    out = device_grid(verts, faces, 5).cast(od[:0], dd[:0], trd[:0])  # R = 0
    assert all(t.numel() == 0 for t in out)


@pytest.mark.parametrize("name", MC.MESHES)
def test_device_against_float64(name):
    verts, faces = MC.mesh(name)[:2]
    grid = device_grid(verts, faces, 5)
    check_against_float64(name, lambda o, d, tr: as_numpy(grid.cast(*dev(o, d, tr))))
    assert grid.G == 5 and meshray.MeshGrid(dev(verts), dev(faces)).G == meshray.default_G(faces.shape[0])


def test_degenerate_rays_and_bad_faces_on_the_device():
    host = MC.build_host()
    verts, faces = MC.cube()
    o, d, tr, _ = MC.degenerate_rays()
    for G in SIZES_G:
        got = as_numpy(device_grid(verts, faces, G).cast(*dev(o, d, tr)))
        MC.check_degenerate(got)
        want = MC.host_cast(host, MC.host_build(host, verts, faces, G), o, d, tr)
        assert MC.same_hits(got, want) and np.array_equal(got["n_tests"], want["n_tests"])
    from test_meshray_host import bad_mesh
    bv, bf, box, n_bad = bad_mesh()
    o, d, tr = MC.mixed_rays("icosphere")
    for G in (1, 5):
        grid = device_grid(bv, bf, G, aabb=box)
        twin = MC.host_build(host, bv, bf, G, aabb=box)
        assert MC.lists_of(grid.cell_start.cpu().numpy(), grid.cell_list.cpu().numpy()) == MC.lists_of(twin["cell_start"], twin["cell_list"])
        got = as_numpy(grid.cast(*dev(o, d, tr)))
        assert MC.same_hits(got, MC.host_cast(host, twin, o, d, tr)) and not np.isin(got["face"], np.arange(n_bad)).any()
    got = as_numpy(device_grid(bv, bf[:4], 5, aabb=box).cast(*dev(o, d, tr)))  # all faces invalid
    assert (got["face"] == -1).all() and (got["n_tests"] == 0).all() and np.array_equal(got["t"], tr[:, 0])
    dup = as_numpy(device_grid(verts, np.concatenate([faces, faces]), 5).cast(*dev(*MC.mixed_rays("cube"))))  # coplanar duplicates: the lower index
    assert MC.same_hits(dup, MC.host_cast(host, MC.host_build(host, verts, faces, 1), *MC.mixed_rays("cube"))) and (dup["face"] < 12).all()


@functools.lru_cache(None)
def sphere_mesh(G=32, r=0.3):
    origin, step = SC.world(G)
    return mesh.marching_cubes(dev(SC.sphere(G, r)), origin=[float(x) for x in origin], step=[float(x) for x in step])


def test_marching_cubes_sphere_against_the_analytic_one():
    """The mesh lies between the balls of radius r - b - sag and r + b (b: 7b's vertex bound, sag = 3 h^2 / (8 (r - b)): a cell's sagitta, as
    tests/test_gpu_zzzzzzmeshsdf.py derives it), so the first hit of a ray lies between its entries into the two balls"""
    G, r = 32, 0.3
    v, f = sphere_mesh(G, r)
    h, b = 1.0 / (G - 1), SC.sphere_bound(G, r)
    sag = 3 * h * h / (8 * (r - b))
    grid = meshray.MeshGrid(v, f)
    for kind, n in (("hit", 128), ("miss", 64)):
        o, d, tr = MC.rays("icosphere", kind, n)
        hits = grid.cast(*dev(o, d, tr))
        got = hits.hit.cpu().numpy()
        assert got.all() if kind == "hit" else not got.any()  # the analytic hit: impact parameter <= 0.8 r, or >= 1.3 r
        if kind == "hit":
            o64, d64 = o.astype(np.float64), d.astype(np.float64)
            ln = np.linalg.norm(d64, axis=1)
            s_c = -(o64 * d64).sum(1) / ln  # metric depth of the closest approach to the centre
            p2 = (o64 ** 2).sum(1) - s_c ** 2
            depth = hits.t.cpu().numpy().astype(np.float64) * ln
            near, far = s_c - np.sqrt((r + b) ** 2 - p2), s_c - np.sqrt((r - b - sag) ** 2 - p2)
            print("marching-cubes sphere, F = %d, G = %d: depth - analytic in [%.3e, %.3e], allowed [%.3e, %.3e]; mean n_tests %.1f"
                  % (f.shape[0], grid.G, (depth - (s_c - np.sqrt(r * r - p2))).min(), (depth - (s_c - np.sqrt(r * r - p2))).max(),
                     (near - (s_c - np.sqrt(r * r - p2))).min(), (far - (s_c - np.sqrt(r * r - p2))).max(), hits.n_tests.float().mean()))
            assert (depth >= near - 1e-6).all() and (depth <= far + 1e-6).all()
            assert bool(hits.front.bool().all())  # the mesher's normals point towards increasing values: outwards
            n = hits.normal(v, f)
            radial = torch.nn.functional.normalize(hits.xyz(v, f), dim=-1)
            assert float((n * radial).sum(-1).min()) > 0.95


def test_ray_range_in_front_of_the_sphere_tracer():
    """the marching-cubes mesh of 7i's analytic "sphere" field (its level-0 lattice), a band of one level-0 cell: trace_surface with the narrowed
    range gives the same hit on every ray, t within 5 eps / len of the unnarrowed trace, and no more evaluations in all"""
    P, cfg = TC.field("sphere")
    Pd = {k: v.to(DEV) for k, v in P.items()}
    r0 = TC.res_list(cfg)[0]
    lo, hi = P["aabb"][0].double().numpy(), P["aabb"][1].double().numpy()
    cell = float((hi - lo)[0] / r0)
    ax = [lo[a] + (hi[a] - lo[a]) * np.arange(r0 + 1) / r0 for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    vol = (np.sqrt(X * X + Y * Y + Z * Z) - 0.08).astype(np.float32)
    v, f = mesh.marching_cubes(dev(vol), origin=[float(x) for x in lo], step=[cell] * 3)
    assert f.shape[0] > 100
    grid = meshray.MeshGrid(v, f)
    o, d, tr = (np.concatenate([TC.rays("sphere", "hit", 128)[i], TC.rays("sphere", "miss", 64)[i]]) for i in range(3))
    od, dd, trd = dev(o, d, tr)
    narrowed, seen = proxy.ray_range(grid, od, dd, trd, band=cell)
    assert bool(seen[:128].all()) and not bool(seen[128:].any())
    assert bool((narrowed[:128, 0] >= trd[:128, 0]).all()) and bool((narrowed[:128, 1] <= trd[:128, 1]).all()) and bool((narrowed[:128, 0] < narrowed[:128, 1]).all())
    assert bool(torch.isneginf(narrowed[128:, 1]).all()) and torch.equal(narrowed[128:, 0], trd[128:, 0])
    plain = hashfield.trace_surface(Pd, cfg, od, dd, trd)
    tight = hashfield.trace_surface(Pd, cfg, od, dd, narrowed)
    assert torch.equal(plain.hit, tight.hit) and bool(plain.hit[:128].all()) and not bool(plain.hit[128:].any())
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    err = np.abs(tight.t.cpu().numpy().astype(np.float64) - plain.t.cpu().numpy())[:128] * ln[:128] / TC.EPS
    n_plain, n_tight = int(plain.n_eval.sum()), int(tight.n_eval.sum())
    print("ray_range, band %.4f: max |t - t_unnarrowed| * len = %.3f eps; n_eval %d -> %d; width of the range * len: %.4f on average"
          % (cell, err.max(), n_plain, n_tight, float(((narrowed[:128, 1] - narrowed[:128, 0]).cpu().numpy() * ln[:128]).mean())))
    assert err.max() <= TC.T_BOUND and n_tight <= n_plain


def test_gradient_of_the_hit_point_in_the_vertices():
    verts, faces = dev(*MC.icosphere())
    verts.requires_grad_(True)
    grid = meshray.MeshGrid(verts, faces, G=5)
    o, d, tr = (np.concatenate([MC.rays("icosphere", "hit", 128)[i], MC.rays("icosphere", "miss", 64)[i]]) for i in range(3))
    od, dd, trd = dev(o, d, tr)
    hits = grid.cast(od, dd, trd)
    assert not hits.t.requires_grad and bool(hits.hit[:128].all()) and not bool(hits.hit[128:].any())
    xyz, n = hits.xyz(verts, faces), hits.normal(verts, faces)
    assert not xyz[128:].any() and not n[128:].any()
    assert float((xyz.detach()[:128] - (od + hits.t[:, None] * dd)[:128]).abs().max()) < 8 * MC.T_BOUND
    g_hit, = torch.autograd.grad(xyz[:128].sum(), verts, retain_graph=True)
    g_miss, = torch.autograd.grad(xyz[128:].sum() + n[128:].sum(), verts, retain_graph=True)
    g_n, = torch.autograd.grad((n[:128] * dd[:128]).sum(), verts)
    assert abs(float(g_hit.sum()) - 3 * 128) < 1e-3 and bool(g_hit.any()) and not bool(g_miss.any())  # the weights of a face add up to 1 per axis
    assert bool(g_n.any()) and bool(torch.isfinite(g_n).all())


def test_graph_capture():
    """repack + cast captured in a torch.cuda.graph at G = 1 (the lists hold every face whatever the vertices do inside the box), the vertices
    moved between replays, each replay against an eager grid built from the moved vertices; building a grid under capture raises"""
    verts, faces = dev(*MC.icosphere())
    box = torch.tensor([[-0.5] * 3, [0.5] * 3], device=DEV)
    grid = meshray.MeshGrid(verts, faces, G=1, aabb=box)
    od, dd, trd = dev(*MC.rays("icosphere", "hit", 128))
    step = lambda: grid.repack().cast(od, dd, trd)  # noqa: E731
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
        verts += torch.tensor([0.02, -0.01, 0.03], device=DEV)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outs]
    fresh = meshray.MeshGrid(verts, faces, G=7, aabb=box).cast(od, dd, trd)
    assert all(torch.equal(a, b) for a, b in zip(replayed[:5], fresh[:5])) and torch.equal(replayed[6], fresh.hit)
    assert not torch.equal(replayed[0], eager0.t) and bool(fresh.hit.all())
    x = torch.zeros(8, device=DEV)
    graph2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="stream capture"):
        with torch.cuda.graph(graph2):
            y = x + 1  # noqa: F841  (the capture is not empty)
            meshray.MeshGrid(verts, faces, G=2)
    torch.cuda.synchronize()
    assert meshray.MeshGrid(verts, faces, G=2).cell_list.numel() >= 1280  # and it still works afterwards


def test_argument_errors_arrive_before_any_launch():
    verts, faces = dev(*MC.cube())
    od, dd, trd = dev(*MC.rays("cube", "hit", 128))
    grid = meshray.MeshGrid(verts, faces, G=2)
    with pytest.raises(RuntimeError, match=r"G = 129 outside \[1, 128\]"):
        meshray.MeshGrid(verts, faces, G=129)
    with pytest.raises(RuntimeError, match=r"aabb must be float32 \(2, 3\)"):
        meshray.MeshGrid(verts, faces, aabb=torch.zeros(6, device=DEV))
    with pytest.raises(RuntimeError, match="hi > lo on every axis"):
        meshray.MeshGrid(verts, faces, aabb=torch.zeros(2, 3, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshray.MeshGrid(verts.cpu(), faces)
    with pytest.raises(RuntimeError, match="disagree"):
        grid.cast(od, dd[:5], trd)
    with pytest.raises(RuntimeError, match="no CPU path"):
        grid.cast(od.cpu(), dd, trd)
    with pytest.raises(RuntimeError, match="disagree"):
        proxy.ray_range(grid, od, dd, trd[:5])
    from lab4d_amd import _lib
    lib = _lib.lib()
    p = _lib.ptr(od)
    rc = lib.lab4d_mesh_raycast(p, p, p, 4, p, 12, p, 200, p, p, p, p, p, p, p, p, _lib.stream())
    assert rc == -1 and "G = 200" in lib.lab4d_last_error().decode()
    rc = lib.lab4d_mesh_raycast(p, p, p, 4, p, 12, p, 2, p, p, p, None, p, p, p, p, _lib.stream())
    assert rc == -1 and "null pointer (t," in lib.lab4d_last_error().decode()
    rc = lib.lab4d_meshgrid_count(p, p, 8, 12, p, 0, p, p, p, p, _lib.stream())
    assert rc == -1 and "G = 0" in lib.lab4d_last_error().decode()
    torch.cuda.synchronize()
