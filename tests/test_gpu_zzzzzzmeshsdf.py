"""The mesh distance on the device (csrc/meshsdf.hip through lab4d_amd/meshsdf.py, proxy.py, occgrid.py and patch.py): the kernels
against the CPU twin (tests/host_harness/meshsdf_host.cpp) -- distance, face and closest point BIT FOR BIT, at every slice count -- on the
meshes of tests/test_meshsdf_host.py, which pins the twin against float64; then the host layer: a marching-cubes mesh, seed_from_mesh,
init_sdf_fn and its opt-in binding, the argument checks and graph capture."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_checks as MC  # noqa: E402
import meshsdf_checks as SC  # noqa: E402

from lab4d_amd import meshsdf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_MAX = 1025


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(None)
def twin_case(F):
    """the first F faces of the 1,280-face icosphere (closed only at F = 1280), 1,025 points random in 1.5 x its box, the twin's answer"""
    verts, faces = SC.icosphere()
    faces = np.ascontiguousarray(faces[:F])
    pts = SC.points_around(verts, N_MAX, seed=F)
    return verts, faces, pts, SC.host_query(SC.build_host(), verts, faces, pts)


def query(verts, faces, pts, **kw):
    sdf, face, closest = meshsdf.signed_distance(dev(verts), dev(faces), dev(pts), return_face=True, return_closest=True, **kw)
    return sdf, face, closest


@pytest.mark.parametrize("F", [0, 1, 255, 256, 257, 1280])
def test_kernels_equal_the_cpu_twin_bit_for_bit(F):
    verts, faces, pts, twin = twin_case(F)
    L = SC.bbox_diagonal(verts, pts)
    far = np.sqrt(twin["d2"]) > 1e-3 * L
    for N in (1, 63, 64, 65, 257, N_MAX):
        first = None
        for n_slices in (1, 2, 3, 7, -(-F // 256) + 2):
            sdf, face, closest = query(verts, faces, pts[:N], n_slices=n_slices)
            assert sdf.shape == (N,) and face.shape == (N,) and closest.shape == (N, 3) and face.dtype == torch.int32
            what = (F, N, n_slices)
            assert np.array_equal(u32(sdf.abs()), np.abs(twin["sdf"][:N]).view(np.uint32)), what
            assert np.array_equal(face.cpu().numpy(), twin["face"][:N]), what
            assert np.array_equal(u32(closest), twin["closest"][:N].view(np.uint32)), what
            if F == 1280:  # closed: the sign is the twin's away from the surface
                assert np.array_equal((sdf < 0).cpu().numpy()[far[:N]], (twin["sdf"][:N] < 0)[far[:N]]), what
            if first is None:
                first = (sdf, face, closest)
            assert torch.equal(sdf.abs(), first[0].abs()) and torch.equal(face, first[1]) and torch.equal(closest, first[2]), what
            again = query(verts, faces, pts[:N], n_slices=n_slices)
            assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(again, (sdf, face, closest))), what  # run to run, the sign included
    if F == 0:
        assert bool(torch.isposinf(sdf).all()) and bool((face == -1).all()) and torch.equal(closest, dev(pts))
    if F == 1280:
        assert 0.1 < float((sdf < 0).float().mean()) < 0.5
        d2 = sdf.double() ** 2  # (sdf^2 is not d2 bit for bit: compared as a distance above, as a square here within its rounding)
        assert float((d2.cpu() - torch.from_numpy(twin["d2"]).double()).abs().max()) <= 4 * SC.EPS32 * float(twin["d2"].max())
    # the default slice count and leading dimensions
    sdf2 = meshsdf.signed_distance(dev(verts), dev(faces), dev(pts[:1024]).reshape(4, 256, 3))
    assert sdf2.shape == (4, 256) and np.array_equal(u32(sdf2.abs()).reshape(-1), np.abs(twin["sdf"][:1024]).view(np.uint32))


def test_edge_cases_on_the_device():
    verts, faces = SC.cube()
    pts = SC.points_around(verts, 300, 5)
    pts[0, 0], pts[1, 1], pts[2, 2], pts[3] = np.nan, np.inf, -np.inf, np.nan
    v2 = np.concatenate([verts, [[np.nan, 0, 0], [np.inf, 1, 2], [0.1, 0.1, 0.1]]]).astype(np.float32)
    bad = np.array([[0, 0, 1], [0, 1, 1], [2, 2, 2], [0, 1, 11], [-1, 2, 3], [0, 1, 8], [9, 1, 2], [2 ** 31 - 1, 0, 1], [0, 6, 6], [10, 10, 3], [0, 1, -2 ** 31]], np.int32)
    mixed = np.concatenate([bad[:5], faces[:7], bad[5:], faces[7:]])
    twin = SC.host_query(SC.build_host(), v2, mixed, pts)
    assert np.isnan(twin["sdf"][:4]).all() and np.isfinite(twin["sdf"][4:]).all()
    for n_slices in (1, 4, 30):
        sdf, face, closest = query(v2, mixed, pts, n_slices=n_slices)
        assert bool(torch.isnan(sdf[:4]).all()) and bool((face[:4] == -1).all()) and np.array_equal(u32(closest[:4]), pts[:4].view(np.uint32))
        assert np.array_equal(u32(sdf[4:]), twin["sdf"][4:].view(np.uint32))  # the cube: the twin's sign too (no point within an ulp of w = 0.5)
        assert np.array_equal(face.cpu().numpy(), twin["face"]) and np.array_equal(u32(closest[4:]), twin["closest"][4:].view(np.uint32))
        # optional outputs left out (NULL in the C call)
        only = meshsdf.signed_distance(dev(v2), dev(mixed), dev(pts), n_slices=n_slices)
        assert torch.is_tensor(only) and np.array_equal(u32(only), u32(sdf))
        # no valid face, no face, no vertex
        for v, f in ((v2, bad), (verts, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), faces)):
            sdf, face, closest = query(v, f, pts, n_slices=n_slices)
            assert bool(torch.isnan(sdf[:4]).all()) and bool(torch.isposinf(sdf[4:]).all()) and bool((face == -1).all())
            assert np.array_equal(u32(closest), pts.view(np.uint32))
    assert meshsdf.signed_distance(dev(verts), dev(faces), torch.zeros(0, 3, device=DEV)).shape == (0,)


@functools.lru_cache(None)
def sphere_mesh(G=32, r=0.3):
    from lab4d_amd import mesh
    origin, step = MC.world(G)
    v, f = mesh.marching_cubes(dev(MC.sphere(G, r)), origin=[float(x) for x in origin], step=[float(x) for x in step])
    return v, f


def sphere_tolerance(G=32, r=0.3):
    """The mesh's vertices lie within b = MC.sphere_bound of the sphere, and a triangle inside one cell (chord at most
    sqrt(3) h) dips at most sag = 3 h^2 / (8 (r - b)) below its vertices: ball(r - b - sag) < inside of the mesh < ball(r + b), and signed
    distances are ordered like the sets, so |sdf - (|p| - r)| <= b + sag."""
    h, b = 1.0 / (G - 1), MC.sphere_bound(G, r)
    return b + 3 * h * h / (8 * (r - b)) + 1e-6


def test_marching_cubes_mesh_of_a_sphere_volume():
    v, f = sphere_mesh()
    assert f.shape[0] > 1000
    pts = dev(SC.points_around(np.array([[-0.5] * 3, [0.5] * 3]), 4096, 3, scale=1.0))
    special = torch.tensor([[0.0, 0.0, 0.0]] + [[sx * 0.5, sy * 0.5, sz * 0.5] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], device=DEV)
    pts = torch.cat([special, pts])
    sdf = meshsdf.signed_distance(v, f, pts)
    err = (sdf.double() - (pts.double().norm(dim=1) - 0.3)).abs().max()
    print("32^3 sphere mesh: F %d, default n_slices %d, max |sdf - (|p| - r)| = %.3e (bound %.3e)" % (f.shape[0], meshsdf.default_slices(pts.shape[0], f.shape[0]),
                                                                                                 float(err), sphere_tolerance()))
    assert float(err) <= sphere_tolerance()
    assert float(sdf[0]) < -0.29 and bool((sdf[1:9] > 0.5).all())
    # every slice count gives the same distances, the twin the same bits
    twin = SC.host_query(SC.build_host(), v.cpu().numpy(), f.cpu().numpy(), pts[:300].cpu().numpy())
    for n in (1, 5):
        got = meshsdf.signed_distance(v, f, pts[:300], n_slices=n)
        assert np.array_equal(u32(got.abs()), np.abs(twin["sdf"]).view(np.uint32)) and torch.equal(got < 0, dev(twin["sdf"] < 0))


@pytest.mark.parametrize("G", [5, 32])
def test_seed_from_mesh_is_conservative(G):
    from lab4d_amd import occgrid
    v, f = sphere_mesh()
    aabb = dev(np.array([[-0.5, -0.45, -0.4], [0.5, 0.45, 0.55]], np.float32))
    pts = dev(SC.points_around(aabb.cpu().numpy(), 4096, G, scale=1.0))
    sdf = meshsdf.signed_distance(v, f, pts)
    for band in (0.0, 0.05):
        grid = occgrid.OccupancyGrid(aabb, G=G, decay=0.5, thresh=0.01)
        assert grid.seed_from_mesh(v, f, band=band) is grid
        n = int(grid.n_occupied)
        assert 0 < n < G ** 3
        inside = sdf <= band
        assert int(inside.sum()) > 100 and bool(grid.mask(pts)[inside].all())
        if G == 32:  # and it is a seed, not a full grid: well outside the margin nothing is set
            cell_diag = float(((aabb[1] - aabb[0]) / G).norm())
            assert not bool(grid.mask(pts)[sdf > band + 1.5 * cell_diag].any())
    # the EMA carries on: ema = 2 thresh + 1 = 1.02 halves per empty update, below thresh = 0.01 after 7
    zeros = torch.zeros(G ** 3, device=DEV)
    for _ in range(6):
        grid.update(zeros)
    assert int(grid.n_occupied) == n
    grid.update(zeros)
    assert int(grid.n_occupied) == 0


def test_init_sdf_fn_and_its_binding():
    import types
    import standins
    from lab4d_amd import mesh, patch, proxy, synthetic
    v, f = sphere_mesh()
    pts = dev(SC.points_around(np.array([[-0.5] * 3, [0.5] * 3]), 256, 9, scale=1.0))
    want = meshsdf.signed_distance(v, f, pts)[:, None]
    for vv, ff in ((v, f), (v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64))):  # tensors, or a trimesh's arrays
        fn = proxy.init_sdf_fn(vv, ff)
        out = fn(pts)
        assert out.shape == (256, 1) and out.dtype == pts.dtype and torch.equal(out, want)
    inside = pts.norm(dim=1) < 0.28
    assert int(inside.sum()) > 5 and bool((out[inside] < 0).all()) and bool((out[pts.norm(dim=1) > 0.32] > 0).all())
    # the opt-in binding on a stand-in field
    P = synthetic.to_device(synthetic.make_weights(2), DEV)
    frames = synthetic.add_codes(synthetic.to_device(synthetic.make_frames(3, 2, 64), DEV), P)
    field = standins.fg_field(P, frames, training=False)
    field.proxy_geometry = mesh.to_mesh_object(v, f)
    assert not hasattr(field, "get_init_sdf_fn")  # the stand-in has no method of its own: the default leaves it alone
    patch.configure(field, precision="f32")
    assert not hasattr(field, "get_init_sdf_fn")
    patch.configure(field, init_sdf="device")
    assert torch.equal(field.get_init_sdf_fn()(pts), want)
    assert not hasattr(field.basefield, "get_init_sdf_fn")  # only modules that carry a mesh
    patch.configure(field, init_sdf="reference")
    assert not hasattr(field, "get_init_sdf_fn") and field._lab4d_amd_init_sdf == "reference"
    with pytest.raises(ValueError):
        patch.configure(field, init_sdf="pysdf")
    # a field class with the reference's method: shadowed on the object, restored by "reference"
    class Field(standins.Node):
        def get_init_sdf_fn(self):
            return "reference"
    fld = Field()
    fld.proxy_geometry = types.SimpleNamespace(vertices=v.cpu().numpy(), faces=f.cpu().numpy())
    assert fld.get_init_sdf_fn() == "reference"
    patch.configure(fld, init_sdf="device")
    assert torch.equal(fld.get_init_sdf_fn()(pts), want) and Field().get_init_sdf_fn() == "reference"
    patch.configure(fld, init_sdf="reference")
    assert fld.get_init_sdf_fn() == "reference"
    fld.proxy_geometry = None
    patch.configure(fld, init_sdf="device")
    with pytest.raises(RuntimeError, match="vertices"):
        fld.get_init_sdf_fn()


def test_arguments_are_checked_before_any_launch_and_the_call_is_capturable():
    from lab4d_amd import _lib
    verts, faces = (dev(a) for a in SC.icosphere())
    pts = dev(SC.points_around(SC.icosphere()[0], 512, 1))
    with pytest.raises(RuntimeError, match="n_slices = 0"):
        meshsdf.signed_distance(verts, faces, pts, n_slices=0)
    with pytest.raises(RuntimeError, match="int64 faces"):
        meshsdf.signed_distance(verts, faces.long(), pts)
    with pytest.raises(RuntimeError, match="work must be float32"):
        meshsdf.signed_distance(verts, faces, pts, n_slices=4, work=torch.empty(10, device=DEV))
    lib = _lib.lib()
    out = torch.full((512,), -7.0, device=DEV)
    args = dict(v=_lib.ptr(verts), f=_lib.ptr(faces), p=_lib.ptr(pts), o=_lib.ptr(out), s=_lib.stream())
    call = lambda nv, nf, n, ns, work, p=args["p"], o=args["o"], f=args["f"]: lib.lab4d_mesh_sdf(args["v"], f, nv, nf, p, n, ns, work, o, None, None, args["s"])  # noqa: E731
    for a, kw, word in (((-1, 1280, 512, 1, None), {}, b"negative"), ((642, 1280, -1, 1, None), {}, b"negative"), ((642, 1280, 512, 0, None), {}, b"n_slices"),
                        ((642, 1280, 512, 70000, None), {}, b"n_slices"), ((642, 1280, 512, 2, None), {}, b"work"), ((642, 2 ** 31 // 3 + 1, 512, 1, None), {}, b"2^31 / 3"),
                        ((642, 1280, 512, 1, None), {"p": None}, b"null"), ((642, 1280, 512, 1, None), {"o": None}, b"null"), ((642, 1280, 512, 1, None), {"f": None}, b"faces"),
                        ((642, 1280, 2 ** 30, 3, None), {}, b"chunks")):
        assert call(*a, **kw) == -1 and word in lib.lab4d_last_error(), (a, kw, lib.lab4d_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing was launched
    assert call(642, 1280, 0, 1, None, p=None, o=None) == 0  # no points: nothing to do
    # capture with the work buffer preallocated and the slice count fixed; replay with the points changed
    n_slices = 3
    work = torch.empty(meshsdf.work_words(512, n_slices), device=DEV)
    buf = pts.clone()
    eager = [meshsdf.signed_distance(verts, faces, p, n_slices=n_slices, return_face=True, return_closest=True, work=work) for p in (pts, -pts)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        got = meshsdf.signed_distance(verts, faces, buf, n_slices=n_slices, return_face=True, return_closest=True, work=work)
    for want, p in zip(eager, (pts, -pts)):
        buf.copy_(p)
        for t in got:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(got, want))
    assert not torch.equal(eager[0][0], eager[1][0])
