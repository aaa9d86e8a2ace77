"""Closest point and signed distance through the face grid on the device (csrc/meshnear.hip through lab4d_amd.meshray.MeshGrid.closest and its
consumers): the kernel against its CPU twin bit for bit (tests/meshnear_checks.py; tests/test_meshnear_host.py pins the twin), against the
brute-force lab4d_amd.meshsdf.signed_distance word for word, a marching-cubes sphere against the analytic one, the consumers' grid keyword, the
gradient of the closest point in the vertices, graph capture and the guards."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_checks as SC  # noqa: E402
import meshnear_checks as NC  # noqa: E402
import meshray_checks as MC  # noqa: E402
import meshsdf_checks as SD  # noqa: E402

from lab4d_amd import mesh, meshray, meshsdf, occgrid, proxy  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES_F = (0, 1, 255, 256, 257, 1280)
SIZES_N = (1, 63, 64, 65, 257, 1025)
KEYS = ("sdf", "d2", "face", "closest", "region", "n_tests")


def dev(*arrays):
    out = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)
    return out[0] if len(out) == 1 else out


def as_numpy(near):
    return {k: getattr(near, k).cpu().numpy() for k in KEYS}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def device_grid(verts, faces, G, aabb=None):
    return meshray.MeshGrid(dev(verts), dev(faces), G=G, aabb=None if aabb is None else dev(np.asarray(aabb, np.float32).reshape(2, 3)))


def twin(verts, faces, pts, G, sign_mode=1, orient=1, aabb=None):
    return NC.host_closest(NC.build_host(), MC.host_build(MC.build_host(), verts, faces, G, aabb=aabb), pts, sign_mode, orient)


def check_against_twin(got, want, what):
    """d2, face, closest, region and n_tests word for word; sdf word for word on face and edge regions, its sign everywhere (the point sets keep
    every compared vertex-region sign off the margin: tests/test_meshnear_host.py asserts it; an on-surface point's sdf is +-0 or a rounding)"""
    bad = [int((bits(got[k]) != bits(want[k])).any()) for k in ("d2", "face", "closest", "region", "n_tests")]
    assert not any(bad), (what, bad)
    flat = want["region"] <= 3
    assert np.array_equal(bits(got["sdf"][flat]), bits(want["sdf"][flat])), what
    assert np.array_equal(bits(np.abs(got["sdf"])), bits(np.abs(want["sdf"]))), what


@functools.lru_cache(None)
def chosen(name):
    """the points of NC.points(name) farther than 1e-5 L from the surface in float64"""
    verts, faces = MC.mesh(name)[:2]
    pts, _ = NC.points(name)
    L = float(np.linalg.norm(np.diff(MC.default_aabb(verts).astype(np.float64), axis=0)))
    return np.sqrt(SD.ref_query(verts, faces, pts)["d2"]) > NC.OFF_SURFACE * L


def test_kernel_against_the_twin_on_the_first_F_faces():
    """F in {0, 1, 255, 256, 257, 1280} (the first F faces of the icosphere in its box), N in {1, 63, 64, 65, 257, 1025}, G in {1, 2, 5, 32}"""
    verts, faces = MC.icosphere()
    box = MC.default_aabb(verts)
    pts, where = NC.points("icosphere")
    pick = np.concatenate([np.arange(where[k].start, where[k].stop)[:n] for k, n in (("inside", 256), ("far1", 64), ("far8", 64), ("far1024", 64), ("verts", 200),
                                                                                    ("edges", 200), ("faces", 113), ("corners5", 64))])
    pts = np.ascontiguousarray(pts[pick][np.random.default_rng(3).permutation(pick.size)])
    assert pts.shape[0] == 1025
    ptd = dev(pts)
    for F in SIZES_F:
        for G in NC.SIZES_G:
            want = twin(verts, faces[:F], pts, G, aabb=box)
            grid = device_grid(verts, faces[:F], G, aabb=box)
            for N in SIZES_N:
                got = as_numpy(grid.closest(ptd[:N], orient=1))
                sl = {k: v[:N] for k, v in want.items()}
                check_against_twin(got, sl, (F, G, N))
                if F == 1280:  # closed: the sign is the twin's on every point off the surface
                    off = chosen("icosphere")[pick][np.random.default_rng(3).permutation(pick.size)][:N]
                    assert np.array_equal(got["sdf"][off] < 0, sl["sdf"][off] < 0), (F, G, N)
    out = device_grid(verts, faces, 5).closest(ptd[:0])  # N = 0
    assert all(t.numel() == 0 for t in out)
    lead = device_grid(verts, faces, 5).closest(ptd[:24].reshape(2, 3, 4, 3))
    assert lead.sdf.shape == (2, 3, 4) and lead.closest.shape == (2, 3, 4, 3) and lead.region.shape == (2, 3, 4)


@pytest.mark.parametrize("name", MC.MESHES)
def test_kernel_against_the_twin_and_brute_force(name):
    """the whole point set of a mesh at every G: == the twin, and == lab4d_amd.meshsdf.signed_distance in |sdf|, face and closest word for word; on
    the closed meshes the sign matches the winding number's at every point farther than 1e-5 L from the surface, in both orientations"""
    verts, faces = MC.mesh(name)[:2]
    pts, _ = NC.points(name)
    vd, fd, ptd = dev(verts, faces, pts)
    sdf_b, face_b, q_b = (t.cpu().numpy() for t in meshsdf.signed_distance(vd, fd, ptd, return_face=True, return_closest=True))
    off = chosen(name)
    for G in NC.SIZES_G:
        grid = meshray.MeshGrid(vd, fd, G=G)
        got = as_numpy(grid.closest(ptd))
        want = twin(verts, faces, pts, G, orient=NC.volume_orient(verts, faces))
        check_against_twin(got, want, (name, G))
        assert np.array_equal(got["sdf"][off] < 0, want["sdf"][off] < 0), (name, G)  # vertex regions included: the sets keep them off the margin
        assert np.array_equal(bits(np.abs(got["sdf"])), bits(np.abs(sdf_b))) and np.array_equal(got["face"], face_b) and np.array_equal(bits(got["closest"]), bits(q_b))
        if name != "hemisphere":
            assert grid.orientation() == 1 and np.array_equal(got["sdf"][off] < 0, sdf_b[off] < 0), (name, G)
        unsigned = as_numpy(grid.closest(ptd, sign=None))
        assert np.array_equal(bits(unsigned["sdf"]), bits(np.abs(got["sdf"]))) and all(np.array_equal(bits(unsigned[k]), bits(got[k])) for k in KEYS[1:])
    if name != "hemisphere":
        flipped = dev(SD.flipped(faces))
        grid = meshray.MeshGrid(vd, flipped, G=5)
        got = as_numpy(grid.closest(ptd))
        assert grid.orientation() == -1 and np.array_equal(got["sdf"][off] < 0, sdf_b[off] < 0)
        assert np.array_equal(as_numpy(grid.closest(ptd, orient=1))["sdf"][off] < 0, sdf_b[off] > 0)  # a fixed +1 on an inward mesh: all flipped


def test_edge_cases_on_the_device():
    verts, faces = MC.cube()
    pts, _ = NC.points("cube")
    nan, inf = np.nan, np.inf
    odd = np.array([[nan, 0, 0], [0, nan, 0], [0, 0, nan], [inf, 0, 0], [0, -inf, 0], [0, 0, inf]], np.float32)
    allp = np.concatenate([pts, odd])
    bv, bf, box, n_bad = NC.bad_cube()
    soup = verts[faces].reshape(-1, 3)
    for G in (1, 5):
        check_against_twin(as_numpy(device_grid(verts, faces, G).closest(dev(allp))), twin(verts, faces, allp, G), ("cube", G))
        got = as_numpy(device_grid(bv, bf, G, aabb=box).closest(dev(allp), orient=1))
        check_against_twin(got, twin(bv, bf, allp, G, aabb=box), ("bad faces", G))
        assert (got["face"][:-6] >= n_bad).all() and np.isnan(got["sdf"][-6:]).all() and (got["face"][-6:] == -1).all()
        assert np.array_equal(bits(got["closest"][-6:]), bits(odd))
        none = as_numpy(device_grid(bv, bf[:n_bad], G, aabb=box).closest(dev(pts)))  # all faces invalid
        assert np.isposinf(none["sdf"]).all() and (none["face"] == -1).all() and np.array_equal(bits(none["closest"]), bits(pts))
        dup = as_numpy(device_grid(verts, np.concatenate([faces, faces]), G).closest(dev(pts)))  # coplanar duplicates: the lower index
        welded = as_numpy(device_grid(verts, faces, G).closest(dev(pts)))
        assert (dup["face"] < 12).all() and all(np.array_equal(bits(dup[k]), bits(welded[k])) for k in KEYS[:5])
        unwelded = as_numpy(device_grid(soup, np.arange(36, dtype=np.int32).reshape(12, 3), G).closest(dev(pts)))
        assert all(np.array_equal(bits(unwelded[k]), bits(welded[k])) for k in KEYS[:5])
    empty = as_numpy(meshray.MeshGrid(dev(verts), dev(faces[:0]), G=4).closest(dev(pts)))  # F = 0
    assert np.isposinf(empty["sdf"]).all() and (empty["face"] == -1).all() and (empty["n_tests"] == 0).all()


@functools.lru_cache(None)
def sphere_mesh(G=32, r=0.3):
    origin, step = SC.world(G)
    return mesh.marching_cubes(dev(SC.sphere(G, r)), origin=[float(x) for x in origin], step=[float(x) for x in step])


def test_marching_cubes_sphere_against_the_analytic_one():
    """The 32^3 mesh lies between the balls of radius r - b - sag and r + b (b: 7b's vertex bound, sag = 3 h^2 / (8 (r - b)): a cell's sagitta, as
    tests/test_gpu_zzzzzzmeshsdf.py derives it): |sdf - (|p| - r)| <= b + sag with the analytic sign at 4,096 random points of the volume on both
    sides of the surface, orient="auto" (the mesher's normals point outward)"""
    G, r = 32, 0.3
    v, f = sphere_mesh(G, r)
    h, b = 1.0 / (G - 1), SC.sphere_bound(G, r)
    sag = 3 * h * h / (8 * (r - b))
    p = np.random.default_rng(5).uniform(-0.5, 0.5, (4096, 3)).astype(np.float32)
    want = np.linalg.norm(p.astype(np.float64), axis=1) - r
    grid = meshray.MeshGrid(v, f)
    got = grid.closest(dev(p))
    sdf = got.sdf.cpu().numpy().astype(np.float64)
    clear = np.abs(want) > b + sag + 1e-6
    print("marching-cubes sphere, F = %d, G = %d, orient %+d: sdf - analytic in [%.3e, %.3e], allowed +-%.3e; mean n_tests %.1f; %d inside, %d outside"
          % (f.shape[0], grid.G, grid.orientation(), (sdf - want).min(), (sdf - want).max(), b + sag + 1e-6, got.n_tests.float().mean(), (want < 0).sum(), (want > 0).sum()))
    assert grid.orientation() == 1 and (want[clear] < 0).sum() > 300 and (want[clear] > 0).sum() > 2000
    assert np.array_equal(sdf[clear] < 0, want[clear] < 0)
    assert (np.abs(np.abs(sdf) - np.abs(want)) <= b + sag + 1e-6).all() and (np.abs(sdf[clear] - want[clear]) <= b + sag + 1e-6).all()


def test_consumers():
    """signed_distance(grid=), init_sdf_fn(grid=True) and seed_from_mesh(grid=) against the grid's own answer and against the brute-force paths"""
    v, f = sphere_mesh()
    p = dev(np.random.default_rng(6).uniform(-0.5, 0.5, (5, 100, 3)).astype(np.float32))
    grid = meshray.MeshGrid(v, f)
    near = grid.closest(p)
    sdf, face, q = meshsdf.signed_distance(v, f, p, return_face=True, return_closest=True, grid=grid)
    assert sdf.shape == (5, 100) and face.shape == (5, 100) and q.shape == (5, 100, 3)
    assert torch.equal(sdf, near.sdf) and torch.equal(face, near.face) and torch.equal(q, near.closest)
    only = meshsdf.signed_distance(v, f, p, grid=grid)
    assert torch.is_tensor(only) and torch.equal(only, near.sdf)
    brute, face_b, q_b = meshsdf.signed_distance(v, f, p, return_face=True, return_closest=True)
    assert torch.equal(sdf.abs(), brute.abs()) and torch.equal(face, face_b) and torch.equal(q, q_b)
    off = brute.abs() > 1e-5 * 3 ** 0.5
    assert torch.equal(sdf[off] < 0, brute[off] < 0)
    with pytest.raises(RuntimeError, match="MeshGrid of this mesh"):
        meshsdf.signed_distance(v, f[:-1].contiguous(), p, grid=grid)
    flat = p.reshape(-1, 3)
    a, b = proxy.init_sdf_fn(v, f, grid=True)(flat), proxy.init_sdf_fn(v, f)(flat)
    assert a.shape == (500, 1) and torch.equal(a.abs(), b.abs()) and torch.equal(a[off.reshape(-1, 1)] < 0, b[off.reshape(-1, 1)] < 0)
    box = torch.tensor([[-0.5] * 3, [0.5] * 3], device=DEV)
    for G in (5, 32):
        seeded, plain = occgrid.OccupancyGrid(box, G=G), occgrid.OccupancyGrid(box, G=G)
        seeded.seed_from_mesh(v, f, band=0.01, grid=grid)
        plain.seed_from_mesh(v, f, band=0.01)
        assert torch.equal(seeded.bits, plain.bits) and int(seeded.n_occupied) == int(plain.n_occupied) and 0 < int(plain.n_occupied) < G ** 3


def test_gradient_of_the_closest_point_in_the_vertices():
    verts, faces = dev(*MC.icosphere())
    verts.requires_grad_(True)
    grid = meshray.MeshGrid(verts, faces, G=5)
    pts = np.concatenate([NC.points("icosphere")[0][:256], np.array([[np.nan, 0, 0], [0, np.inf, 0]], np.float32)])
    near = grid.closest(dev(pts))
    assert not near.sdf.requires_grad and bool((near.face[:256] >= 0).all()) and bool((near.face[256:] < 0).all())
    xyz = near.xyz(verts, faces)
    assert not xyz[256:].any() and float((xyz.detach()[:256] - near.closest[:256]).abs().max()) < 1e-6
    g_hit, = torch.autograd.grad(xyz[:256].sum(), verts, retain_graph=True)
    g_miss, = torch.autograd.grad(xyz[256:].sum(), verts)
    assert abs(float(g_hit.sum()) - 3 * 256) < 1e-3 and bool(g_hit.any()) and not bool(g_miss.any())  # the weights of a face add up to 1 per axis


def test_graph_capture():
    """closest captured in a torch.cuda.graph and replayed with the points changed in place: equal to eager; orient="auto" that is not cached yet is
    refused under capture"""
    verts, faces = dev(*MC.icosphere())
    grid = meshray.MeshGrid(verts, faces, G=5)
    allp = dev(NC.points("icosphere")[0])
    pts = allp[:512].clone()
    x = torch.zeros(8, device=DEV)
    graph0 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="before the stream capture"):
        with torch.cuda.graph(graph0):
            y = x + 1  # noqa: F841  (the capture is not empty)
            grid.closest(pts)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager0 = grid.closest(pts)  # (caches the orientation)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = grid.closest(pts)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, eager0))
    pts.copy_(allp[512:1024])
    graph.replay()
    torch.cuda.synchronize()
    fresh = grid.closest(allp[512:1024].contiguous())
    assert all(torch.equal(a, b) for a, b in zip(outs, fresh)) and not torch.equal(outs.sdf, eager0.sdf)


def test_guards_and_argument_errors_arrive_before_any_launch():
    verts, faces = dev(*MC.cube())
    pts = dev(NC.points("cube")[0][:64])
    small = torch.tensor([[-0.25] * 3, [0.25] * 3], device=DEV)
    with pytest.raises(RuntimeError, match="does not contain the mesh's vertices"):
        meshray.MeshGrid(verts, faces, G=2, aabb=small).closest(pts)
    grid = meshray.MeshGrid(verts, faces, G=2)
    assert grid._facts is None and grid.closest(pts).sdf.shape == (64,) and grid._facts == (1, True)
    assert grid.rebuild()._facts is None
    with pytest.raises(RuntimeError, match="neither 'pseudonormal' nor None"):
        grid.closest(pts, sign="winding")
    with pytest.raises(RuntimeError, match=r"is not 'auto', \+1 or -1"):
        grid.closest(pts, orient=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        grid.closest(pts.cpu())
    from lab4d_amd import _lib
    lib = _lib.lib()
    p = _lib.ptr(pts)
    for args, msg in (((p, 4, p, 12, p, 200, p, p, 1, 1, p, p, p, p, p, p), "G = 200"), ((p, 4, p, 12, p, 2, p, p, 2, 1, p, p, p, p, p, p), "sign_mode = 2"),
                      ((p, 4, p, 12, p, 2, p, p, 1, 0, p, p, p, p, p, p), "orient = 0"), ((p, -1, p, 12, p, 2, p, p, 1, 1, p, p, p, p, p, p), "N = -1"),
                      ((p, 4, None, 12, p, 2, p, p, 1, 1, p, p, p, p, p, p), "null pointer (tris"), ((p, 4, p, 12, None, 2, p, p, 1, 1, p, p, p, p, p, p), "null pointer (aabb"),
                      ((p, 4, p, 12, p, 2, p, p, 1, 1, None, p, p, p, p, p), "null pointer (pts, sdf"), ((None, 4, p, 12, p, 2, p, p, 1, 1, p, p, p, p, p, p), "null pointer (pts, sdf")):
        assert lib.lab4d_mesh_closest(*args, _lib.stream()) == -1 and msg in lib.lab4d_last_error().decode(), msg
    sdf = torch.empty(64, device=DEV)
    _lib.call("mesh_closest", pts, 64, grid.tris, 12, grid.aabb, 2, grid.cell_start, grid.cell_list, 1, 1, sdf, None, None, None, None, None)  # the optional outputs left out
    assert torch.equal(sdf, grid.closest(pts).sdf)
    torch.cuda.synchronize()
