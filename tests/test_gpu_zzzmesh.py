"""Iso-surface extraction on the device (lab4d_amd/mesh.py, csrc/mesh.hip): the kernels against their CPU twin
(tests/host_harness/mesh_host.cpp: counts and faces bit-equal, vertices bit-equal in index space), the mesh properties of
tests/mesh_checks.py directly on the device output at 64^3 / 128^3, the largest-component filter, the opt-in binding of
NeRF.extract_canonical_mesh, and recorded (not gated) timings."""
import json
import os
import sys
import time
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_checks as MC  # noqa: E402

from lab4d_amd import synthetic  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = MC.ROOT


@pytest.fixture(scope="module")
def host():
    return MC.build_host()


def dev_extract(vol, mask=None, level=0.0, origin=None, step=None, largest_component=False):
    from lab4d_amd import mesh
    kw = {} if origin is None else {"origin": [float(x) for x in origin], "step": [float(x) for x in step]}
    v, f = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, np.float32)).to(DEV), None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).to(DEV),
                               level=level, largest_component=largest_component, **kw)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return v.cpu().numpy(), f.cpu().numpy()


def compare(host, vol, mask=None, level=0.0, G_world=None):
    """device vs CPU twin on one volume: index space bit for bit; world space faces bit for bit, vertices within 2 ulp of the largest box
    coordinate (the licence for a fused multiply-add in origin + step * x)."""
    hv, hf = MC.host_extract(host, vol, mask, level)
    dv, df = dev_extract(vol, mask, level)
    print("volume %s level %g mask %s: V %d F %d" % (vol.shape, level, mask is not None, hv.shape[0], hf.shape[0]))
    assert dv.shape == hv.shape and df.shape == hf.shape, (dv.shape, hv.shape, df.shape, hf.shape)
    assert np.array_equal(df, hf)
    assert np.array_equal(dv.view(np.uint32), hv.view(np.uint32))
    if G_world is not None:
        origin, step = MC.world(G_world)
        hv, hf = MC.host_extract(host, vol, mask, level, origin, step)
        dv, df = dev_extract(vol, mask, level, origin, step)
        assert np.array_equal(df, hf) and dv.shape == hv.shape
        err = float(np.abs(dv - hv).max()) if hv.size else 0.0
        print("   world-space max |device - host| = %.3e (2 ulp of 0.5 = %.3e)" % (err, 2 * np.spacing(np.float32(0.5))))
        assert err <= 2 * np.spacing(np.float32(0.5))
    return dv, df


def test_device_equals_the_cpu_twin_on_the_cpu_suite_volumes(host):
    compare(host, MC.random_volume((14, 14, 14), 5))
    compare(host, MC.random_volume((9, 12, 17), 1))
    G = 32
    sph = MC.sphere(G, 0.3)
    compare(host, sph, G_world=G)
    compare(host, MC.torus(G), G_world=G)
    compare(host, MC.two_spheres(G), G_world=G)
    compare(host, MC.three_blobs(G), G_world=G)
    X, _, _ = MC.grid_xyz(G)
    compare(host, sph, mask=(X < 0.05), G_world=G)
    bad = sph.copy()
    bad[16, 16, 25] = np.nan
    v, _ = compare(host, bad, G_world=G)
    assert np.isfinite(v).all()
    compare(host, sph, level=0.005, G_world=G)
    for vol in (np.ones((7, 8, 9), np.float32), -np.ones((7, 8, 9), np.float32), np.ones((1, 1, 1), np.float32), np.ones((5, 1, 4), np.float32)):
        v, f = dev_extract(vol)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def pick_sdf_bias(seed, kind="fg"):
    """A bias of the sdf head that puts the zero level set inside the box: minus the median of the unbiased field on a coarse grid,
    evaluated by the CPU oracle (the random-init field is nearly constant, so any fixed bias would leave the volume all-in or all-out)."""
    from lab4d_amd import deformable as DF
    from lab4d_amd import proxy
    from oracle import lab4d_oracle as O
    Pc = synthetic.make_weights(seed, sdf_bias=0.0)
    pts = proxy.sample_grid(DF.extend_aabb(Pc["aabb"], 0.5), 12)
    code = Pc["basefield.inst_embedding.mapping.weight"].mean(0, keepdim=True)
    with torch.no_grad():
        sdf = O.nerf_forward(Pc, pts[None], {"basefield": code}, with_color=False, get_density=False)[0, :, 0]
    return -float(sdf.median())


def test_device_equals_the_cpu_twin_on_a_field_volume(host):
    """The real thing: proxy.grid_query at 64^3 on a synthetic field whose level set is non-empty, with and without the visibility mask."""
    from lab4d_amd import mlp, proxy
    seed = 2
    bias = pick_sdf_bias(seed)
    P = synthetic.to_device(synthetic.make_weights(seed, sdf_bias=bias), DEV)
    sdf, vis, box = proxy.grid_query(P, P["aabb"], 64, prec=mlp.PREC_F32)
    vol, m = sdf.cpu().numpy(), vis.cpu().numpy()
    print("field volume: sdf in [%.4f, %.4f], bias %.5f, visible fraction %.3f" % (vol.min(), vol.max(), bias, m.mean()))
    _, f = compare(host, vol)
    assert f.shape[0] > 0
    compare(host, vol, mask=m)
    compare(host, vol, level=0.005)
    # proxy.extract_mesh = the same volume through the public entry point, box transform on the device
    for exact in (False, True):
        v, f, bounds = proxy.extract_mesh(P, P["aabb"], 64, prec=mlp.PREC_F32, use_visibility=False, exact_spacing=exact)
        step = ((box[1] - box[0]) / (63.0 if exact else 64.0)).cpu().numpy()
        hv, hf = MC.host_extract(host, vol, None, 0.0, box[0].cpu().numpy(), step)
        assert np.array_equal(f.cpu().numpy(), hf)
        lim = 2 * np.spacing(np.float32(np.abs(box.cpu().numpy()).max()))
        assert np.abs(v.cpu().numpy() - hv).max() <= lim
        assert torch.equal(bounds, torch.stack([v.min(0)[0], v.max(0)[0]]))
    far = (box[0] + 63 * (box[1] - box[0]) / 64.0)
    v0, _, b0 = proxy.extract_mesh(P, P["aabb"], 64, prec=mlp.PREC_F32, use_visibility=False)
    assert bool((b0[1] <= far + 1e-6).all())  # the reference's 1 / G spacing: nothing reaches the far face of the box


def torch_assert_closed(verts, faces):
    """closed + manifold + consistently oriented, with torch ops on the device: the sorted directed-edge keys have no repeat and equal the
    sorted keys of the reversed edges."""
    V = verts.shape[0]
    f = faces.long()
    assert int(f.min()) >= 0 and int(f.max()) < V
    assert not bool(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).any())
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    key = (e[:, 0] * V + e[:, 1]).sort()[0]
    rkey = (e[:, 1] * V + e[:, 0]).sort()[0]
    assert bool((key[1:] != key[:-1]).all()), "a directed edge occurs twice"
    assert torch.equal(key, rkey), "an edge without its reverse"
    assert torch.equal(torch.unique(f), torch.arange(V, device=f.device))


def torch_euler(verts, faces):
    assert faces.shape[0] % 2 == 0
    return verts.shape[0] - faces.shape[0] // 2  # closed: E = 3 F / 2


def torch_signed_volume(verts, faces):
    t = verts.double()[faces.long()]
    return float((t[:, 0] * torch.cross(t[:, 1], t[:, 2], dim=-1)).sum() / 6)


@pytest.mark.parametrize("G", [64, 128])
def test_properties_hold_on_the_device_output(G):
    from lab4d_amd import mesh
    origin, step = MC.world(G)
    o, s = [float(x) for x in origin], [float(x) for x in step]
    sph = torch.from_numpy(MC.sphere(G, 0.3)).to(DEV)
    v, f = mesh.marching_cubes(sph, origin=o, step=s)
    assert mesh.LAST["readbacks"] == 1  # the two sizes, once
    torch_assert_closed(v, f)
    assert torch_euler(v, f) == 2 and torch_signed_volume(v, f) > 0
    err = float((v.double().norm(dim=1) - 0.3).abs().max())
    print("G %d sphere: V %d F %d, max | |p| - r | %.3e (bound %.3e)" % (G, v.shape[0], f.shape[0], err, MC.sphere_bound(G, 0.3)))
    assert err <= MC.sphere_bound(G, 0.3)
    v, f = mesh.marching_cubes(sph, level=0.005, origin=o, step=s)
    assert float((v.double().norm(dim=1) - 0.305).abs().max()) <= MC.sphere_bound(G, 0.3)
    v, f = mesh.marching_cubes(torch.from_numpy(MC.torus(G)).to(DEV), origin=o, step=s)
    torch_assert_closed(v, f)
    assert torch_euler(v, f) == 0
    v, f = mesh.marching_cubes(torch.from_numpy(MC.two_spheres(G)).to(DEV), origin=o, step=s)
    torch_assert_closed(v, f)
    assert torch_euler(v, f) == 4
    shape = (G, G // 2 + 3, G - 5)
    rv = torch.from_numpy(MC.random_volume(shape, G)).to(DEV)
    v, f = mesh.marching_cubes(rv)
    torch_assert_closed(v, f)
    ins = rv < 0
    n_crossed = sum(int((ins.narrow(a, 0, shape[a] - 1) != ins.narrow(a, 1, shape[a] - 1)).sum()) for a in range(3))
    assert v.shape[0] == n_crossed
    assert bool((((v == v.round()).sum(1)) >= 2).all())


@pytest.mark.parametrize("G", [32, 64])
def test_largest_component(host, G):
    from lab4d_amd import mesh
    origin, step = MC.world(G)
    for name, vol, keep in (("two spheres", MC.two_spheres(G), lambda v: v[:, 0] < 0.04), ("three blobs (tie)", MC.three_blobs(G), lambda v: v[:, 0] < -0.1)):
        v, f = dev_extract(vol, origin=origin, step=step)
        lv, lf = dev_extract(vol, origin=origin, step=step, largest_component=True)
        print("%s G %d: %d -> %d vertices, %d label passes, %d read-backs" % (name, G, v.shape[0], lv.shape[0], mesh.LAST["label_passes"], mesh.LAST["readbacks"]))
        k = keep(v)
        assert 0 < k.sum() < v.shape[0]
        assert np.array_equal(lv, v[k])  # the defined winner's vertices, in their original order
        assert np.array_equal(lv[lf], v[f[k[f[:, 0]]]])
        MC.assert_closed(lv, lf)
        assert MC.euler(lv, lf) == 2
        hv, hf = MC.host_largest_component(host, v, f)
        assert np.array_equal(lv, hv) and np.array_equal(lf, hf)
    if G == 32:  # the tie is genuine
        v, _ = dev_extract(MC.three_blobs(G), origin=origin, step=step)
        assert (v[:, 0] < -0.1).sum() == (v[:, 0] > 0.1).sum()
    # a connected mesh comes back unchanged
    v, f = dev_extract(MC.torus(G), origin=origin, step=step)
    lv, lf = dev_extract(MC.torus(G), origin=origin, step=step, largest_component=True)
    assert np.array_equal(v, lv) and np.array_equal(f, lf)


def test_opt_in_binding_meshes_on_the_device():
    """patch.configure(field, mesher="device"): NeRF.extract_canonical_mesh returns a mesh object built from proxy.extract_mesh without
    calling geom_utils.marching_cubes, and the bound updates accept it."""
    import standins
    from lab4d_amd import mesh, patch, proxy
    seed = 2
    P = synthetic.to_device(synthetic.make_weights(seed, sdf_bias=pick_sdf_bias(seed)), DEV)
    frames = synthetic.add_codes(synthetic.to_device(synthetic.make_frames(seed + 1, 2, 64), DEV), P)
    field = standins.fg_field(P, frames, training=False)
    field.aabb = P["aabb"].clone()
    field.category = "fg"
    patch.configure(field, precision="f32", mesher="device")

    def refuse(*a, **k):
        raise AssertionError("geom_utils.marching_cubes must not be called with mesher='device'")
    saved = {k: sys.modules.get(k) for k in ("lab4d", "lab4d.utils", "lab4d.utils.geom_utils")}
    geom = types.ModuleType("lab4d.utils.geom_utils")
    geom.marching_cubes = refuse
    for k in ("lab4d", "lab4d.utils"):
        sys.modules.setdefault(k, types.ModuleType(k))
    sys.modules["lab4d.utils.geom_utils"] = geom
    try:
        out = patch.nerf_extract_canonical_mesh(field, grid_size=48, level=0.005, use_visibility=False)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    from lab4d_amd import mlp
    v, f, bounds = proxy.extract_mesh(P, field.aabb, 48, level=0.005, prec=mlp.PREC_F32, use_visibility=False, largest_component=True)
    assert f.shape[0] > 0
    assert isinstance(out.vertices, np.ndarray) and isinstance(out.faces, np.ndarray)
    assert np.array_equal(np.asarray(out.vertices, np.float32), v.cpu().numpy()) and np.array_equal(np.asarray(out.faces), f.cpu().numpy())
    assert np.array_equal(np.asarray(out.bounds, np.float32), bounds.cpu().numpy())
    if not isinstance(out, mesh.Mesh):
        import trimesh
        assert isinstance(out, trimesh.Trimesh)
    # the bound updates read .bounds / .vertices of that object
    field.proxy_geometry = out
    before = field.aabb.clone()
    patch.nerf_update_aabb(field)
    assert torch.allclose(field.aabb, proxy.update_aabb(before, bounds), rtol=1e-6, atol=1e-7)
    T = 5
    g = torch.Generator().manual_seed(0)
    quat = torch.nn.functional.normalize(torch.randn(T, 4, generator=g) * 0.1 + torch.tensor([1.0, 0, 0, 0]), dim=-1).to(DEV)
    trans = (torch.randn(T, 3, generator=g) * 0.05 + torch.tensor([0.0, 0.0, 3.0])).to(DEV)
    fm = torch.arange(T, device=DEV)
    nf0 = torch.tensor([[1.0, 5.0]], device=DEV).repeat(T, 1)
    field.near_far = torch.nn.Parameter(nf0.clone(), requires_grad=False)
    field.camera_mlp = types.SimpleNamespace(get_vals=lambda: (quat, trans), time_embedding=types.SimpleNamespace(frame_mapping=fm))
    patch.nerf_update_near_far(field)
    assert torch.allclose(field.near_far.data, proxy.update_near_far(nf0, fm, v, quat, trans), rtol=1e-6, atol=1e-7)
    assert bool(torch.isfinite(field.near_far.data).all()) and not torch.equal(field.near_far.data, nf0)
    # switching back restores the reference's mesher
    patch.configure(field, mesher="reference")
    assert field._lab4d_amd_mesher == "reference"
    with pytest.raises(ValueError):
        patch.configure(field, mesher="skimage")


def test_cpu_tensors_stream_capture_and_bad_arguments_are_refused():
    import ctypes
    from lab4d_amd import _lib, mesh
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.marching_cubes(torch.zeros(4, 4, 4))
    vol = torch.from_numpy(MC.sphere(16, 0.3)).to(DEV)
    with pytest.raises(RuntimeError, match="float32"):
        mesh.marching_cubes(vol.double())
    with pytest.raises(RuntimeError, match="mask"):
        mesh.marching_cubes(vol, mask=torch.ones(4, 4, 4, dtype=torch.bool, device=DEV))
    x = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="stream capture"):
        with torch.cuda.graph(graph):
            y = x + 1  # noqa: F841  (the capture is not empty)
            mesh.marching_cubes(vol)
    torch.cuda.synchronize()
    v, f = mesh.marching_cubes(vol)  # and it still works afterwards
    assert f.shape[0] > 0
    lib = _lib.lib()
    work = torch.zeros(int(lib.lab4d_mesh_work_ints(16, 16, 16)), dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    assert lib.lab4d_mesh_count(None, None, 16, 16, 16, 0.0, _lib.ptr(work), _lib.ptr(counts), _lib.stream()) == -1
    assert lib.lab4d_mesh_count(_lib.ptr(vol), None, 16, 0, 16, 0.0, _lib.ptr(work), _lib.ptr(counts), _lib.stream()) == -1
    assert lib.lab4d_mesh_count(_lib.ptr(vol), None, 1024, 1024, 1024, 0.0, _lib.ptr(work), _lib.ptr(counts), _lib.stream()) == -1
    assert b"too large" in lib.lab4d_last_error()
    torch.cuda.synchronize()
    assert counts.tolist() == [-7, -7]  # nothing was launched
    assert int(lib.lab4d_mesh_work_ints(1024, 1024, 1024)) == -1
    stats = (ctypes.c_int * 2)()
    assert lib.lab4d_mesh_largest_component(None, None, -1, 0, _lib.ptr(work), None, None, _lib.ptr(counts), stats, _lib.stream()) == -1


def _median_ms(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3)


@pytest.mark.parametrize("G", [64, 128, 256])
def test_extraction_times_are_recorded(G):
    """Recorded, not gated (there is no parent-commit time and no skimage to race): extraction alone and grid_query + extraction, a
    random-init field and the sphere, with and without the component filter; median of 5 after 2 warm-ups -> mesh_extract_<G>.json in
    the results directory (tests/mesh_checks.py results_dir)."""
    from lab4d_amd import mesh, proxy
    seed = 2
    P = synthetic.to_device(synthetic.make_weights(seed, sdf_bias=pick_sdf_bias(seed)), DEV)
    sdf, vis, box = proxy.grid_query(P, P["aabb"], G)
    sdf = sdf.contiguous()
    sph = torch.from_numpy(MC.sphere(G, 0.3)).to(DEV)
    res = {"grid": G}
    for name, vol in (("field", sdf), ("sphere", sph)):
        for cc in (False, True):
            key = "%s%s" % (name, "_largest_component" if cc else "")
            ms = _median_ms(lambda: mesh.marching_cubes(vol, largest_component=cc))
            v, f = mesh.marching_cubes(vol, largest_component=cc)
            res[key] = {"extract_ms": ms, "n_verts": int(v.shape[0]), "n_faces": int(f.shape[0]), "label_passes": mesh.LAST["label_passes"],
                        "host_readbacks": mesh.LAST["readbacks"]}
            if not cc:
                assert mesh.LAST["readbacks"] == 1  # extraction alone: the two sizes, once
            assert f.shape[0] > 0
    res["grid_query_ms"] = _median_ms(lambda: proxy.grid_query(P, P["aabb"], G))
    for cc in (False, True):
        res["grid_query_plus_extract%s_ms" % ("_largest_component" if cc else "")] = _median_ms(
            lambda: proxy.extract_mesh(P, P["aabb"], G, largest_component=cc))
    out = MC.results_dir()
    json.dump(res, open(os.path.join(out, "mesh_extract_%d.json" % G), "w"), indent=1)
    print(json.dumps(res))
