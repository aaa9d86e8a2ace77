"""Ray casting against a triangle mesh on the CPU: the twin of the kernels (tests/host_harness/meshray/meshray_host.cpp, the same
csrc/meshray_math.hpp functions) against numpy float64 Moeller-Trumbore over all faces (tests/meshray_checks.py), the independence of the
result from the grid, watertightness, the cell lists against a numpy restatement of the padded-box rule, the degenerate rays, the stand-alone
sanitizer run, the code-object metadata and the argument checks of the Python layer and of the C ABI.  The GPU suite
(tests/test_gpu_zzzzzzzzzzzmeshray.py) holds the kernels to this twin bit for bit.  CPU only.

Measured, twin against float64, max |t - t64| * len over the HIT, MISS and INSIDE sets (128 + 64 + 64 rays) at G = 5: cube 4.85e-7, icosphere
1.13e-7, hemisphere 2.01e-7; bound 4 x the largest = 1.94e-6 (meshray_checks.T_BOUND).  Watertightness: see test_watertight."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import meshray_checks as MC  # noqa: E402

import lab4d_amd.meshray as meshray  # noqa: E402  (the feature under test: its host layer must import without a GPU)

N_HIT, N_MISS, N_INSIDE = 128, 64, 64
G_TRUTH = 5


@pytest.fixture(scope="module")
def host():
    return MC.build_host()


def ray_sets(name):
    return [MC.rays(name, "hit", N_HIT), MC.rays(name, "miss", N_MISS), MC.rays(name, "inside", N_INSIDE)]


def check_against_float64(name, cast):
    """shared with the GPU suite: cast(o, d, tr) -> dict.  hit equal on every ray; |t - t64| len within the bound; the face float64's wherever its
    runner-up is farther away than the bound.  Returns the worst |t - t64| * len."""
    verts, faces, centre, r_in, r_out = MC.mesh(name)
    worst = 0.0
    for kind, (o, d, tr) in zip(("hit", "miss", "inside"), ray_sets(name)):
        b = MC.impact(o, d, centre)
        left_out = (b > 0.8 * r_in) & (b < 1.3 * r_out) if kind != "inside" else np.zeros(len(b), bool)
        assert left_out.mean() == 0
        ref, got = MC.truth(verts, faces, o, d, tr), cast(o, d, tr)
        assert np.array_equal(got["face"] >= 0, ref["hit"]), (name, kind, np.nonzero((got["face"] >= 0) != ref["hit"])[0][:8])
        if kind == "miss":
            assert not ref["hit"].any()
        elif name != "hemisphere":
            assert ref["hit"].all()
        else:
            assert 0.3 < ref["hit"].mean() <= 1.0
        h = ref["hit"]
        ln = np.linalg.norm(d.astype(np.float64), axis=1)
        err = np.abs(got["t"].astype(np.float64) - ref["t"])[h] * ln[h]
        if h.any():
            worst = max(worst, float(err.max()))
            print("%s %s: max |t - t64| * len = %.3e over %d hits" % (name, kind, err.max(), h.sum()))
            assert err.max() <= MC.T_BOUND, (name, kind, err.max())
        clear = h & ((ref["runner_up"] - ref["t"]) * ln > MC.T_BOUND)
        assert np.array_equal(got["face"][clear], ref["face"][clear]) and clear.sum() >= h.sum() // 2, (name, kind, clear.sum(), h.sum())
        assert np.array_equal(got["front"][clear] == 1, ref["front"][clear])
        assert np.array_equal(got["t"][~h], tr[~h, 0]) and not got["u"][~h].any() and not got["v"][~h].any() and not got["front"][~h].any()
        # the barycentric weights give the hit point back
        tri = verts.astype(np.float64)[faces[got["face"][h]]]
        p = tri[:, 0] + got["u"][h, None] * (tri[:, 1] - tri[:, 0]) + got["v"][h, None] * (tri[:, 2] - tri[:, 0])
        q = o[h].astype(np.float64) + got["t"][h, None].astype(np.float64) * d[h]
        assert np.abs(p - q).max() <= 8 * MC.T_BOUND if h.any() else True
    return worst


@pytest.mark.parametrize("name", MC.MESHES)
def test_twin_against_float64(host, name):
    verts, faces = MC.mesh(name)[:2]
    grid = MC.host_build(host, verts, faces, G_TRUTH)
    check_against_float64(name, lambda o, d, tr: MC.host_cast(host, grid, o, d, tr))


@pytest.mark.parametrize("name", MC.MESHES)
def test_grid_independence(host, name):
    """t, face, u, v and front at G = 2, 5, 32 equal G = 1 word for word on every ray of every set, and on the degenerate rays"""
    verts, faces = MC.mesh(name)[:2]
    sets = ray_sets(name) + [MC.mixed_rays(name), MC.degenerate_rays()[:3]]
    base = MC.host_build(host, verts, faces, 1)
    want = [MC.host_cast(host, base, *s) for s in sets]
    assert (want[0]["n_tests"] <= faces.shape[0]).all() and (want[0]["n_tests"][want[0]["face"] >= 0] == faces.shape[0]).all()  # G = 1: brute force
    for G in (2, 5, 32):
        grid = MC.host_build(host, verts, faces, G)
        for s, w in zip(sets, want):
            got = MC.host_cast(host, grid, *s)
            assert MC.same_hits(got, w), (name, G, [int((got[k] != w[k]).sum()) for k in ("t", "face", "u", "v", "front")])
        print("%s G = %d: mean n_tests %.1f (G = 1: %.1f)" % (name, G, got["n_tests"].mean(), want[-1]["n_tests"].mean()))


def mt32_hit(verts, faces, o, d):
    """a plain Moeller-Trumbore test in float32 (any hit, t > 0): what watertightness is measured against"""
    tri = verts[faces]
    a, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    oo, dd = o[:, None], d[:, None]
    h = np.cross(dd, e2).astype(np.float32)
    det = (e1 * h).sum(-1, dtype=np.float32)
    sv = oo - a
    with np.errstate(all="ignore"):
        u = (sv * h).sum(-1, dtype=np.float32) / det
        q = np.cross(sv, e1).astype(np.float32)
        v = (dd * q).sum(-1, dtype=np.float32) / det
        t = (e2 * q).sum(-1, dtype=np.float32) / det
    return ((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)).any(1)


def watertight_rays():
    """8 outside origins x every vertex and every edge midpoint of the icosphere, the targets rounded to fp32"""
    verts, faces = MC.icosphere()
    edges = np.unique(np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1), axis=0)
    targets = np.concatenate([verts, ((verts[edges[:, 0]].astype(np.float64) + verts[edges[:, 1]]) / 2).astype(np.float32)])
    origins = np.array([[sx * 0.9, sy * 0.8, sz * 1.1] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    o = np.repeat(origins, targets.shape[0], 0)
    d = (np.tile(targets, (8, 1)) - o).astype(np.float32)
    tr = np.tile(np.array([[0, 2]], np.float32), (o.shape[0], 1))
    # a target is ON THE SILHOUETTE of its origin when the faces around it (2 at an edge, 5 or 6 at a vertex) do not all face the same way:
    # there the exact ray touches the solid in one point, and the rounding of d = target - o to fp32 decides whether the ray it becomes hits
    tri = verts.astype(np.float64)[faces]
    nrm, cen = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), tri.mean(1)
    around = [[] for _ in range(targets.shape[0])]
    edge_id = {tuple(e): verts.shape[0] + i for i, e in enumerate(edges)}
    for f, (a, b, c) in enumerate(faces):
        for t in (a, b, c, edge_id[(min(a, b), max(a, b))], edge_id[(min(b, c), max(b, c))], edge_id[(min(c, a), max(c, a))]):
            around[t].append(f)
    silhouette = []
    for og in origins.astype(np.float64):
        facing = ((og - cen) * nrm).sum(1) > 0
        silhouette += [len(set(facing[fs])) > 1 for fs in around]
    return o, d, tr, np.array(silhouette)


def test_watertight(host):
    """Every ray aimed at a vertex or an edge midpoint that is not on its origin's silhouette hits, at every G.  The 832 silhouette targets (of
    20,496: every origin's silhouette IS a chain of mesh edges) are left to the rounding of d: float64 Moeller-Trumbore over the same fp32 rays
    misses 360 of them, this test 168, a float32 Moeller-Trumbore 106; off the silhouette none of the three misses any (measured here)."""
    verts, faces = MC.icosphere()
    o, d, tr, silhouette = watertight_rays()
    assert o.shape[0] == 8 * (642 + 1920) and 0 < silhouette.sum() < o.shape[0] // 20
    plain = ~np.concatenate([mt32_hit(verts, faces, o[s:s + 512], d[s:s + 512]) for s in range(0, o.shape[0], 512)])
    for G in (1, 5, 32):
        missed = MC.host_cast(host, MC.host_build(host, verts, faces, G), o, d, tr)["face"] < 0
        print("G = %d: %d rays, %d silhouette targets; missed off the silhouette: %d (float32 Moeller-Trumbore %d), on it: %d (%d)"
              % (G, o.shape[0], silhouette.sum(), (missed & ~silhouette).sum(), (plain & ~silhouette).sum(), (missed & silhouette).sum(), (plain & silhouette).sum()))
        assert not (missed & ~silhouette).any()


def bad_mesh():
    """the icosphere with faces that must not be listed: an index out of range, a negative index, a NaN vertex, a degenerate face, a face outside the box"""
    verts, faces = MC.icosphere()
    box = MC.default_aabb(verts)
    extra_v = np.array([[np.nan, 0, 0], [2, 2, 2], [2.5, 2, 2], [2, 2.5, 2]], np.float32)
    V = verts.shape[0]
    extra_f = np.array([[0, 1, V + 9], [-1, 1, 2], [0, 1, V], [5, 5, 6], [V + 1, V + 2, V + 3]], np.int32)
    return np.concatenate([verts, extra_v]), np.concatenate([extra_f, faces]), box, len(extra_f)


@pytest.mark.parametrize("G", [1, 2, 5, 32])
def test_grid_lists(host, G):
    for name in MC.MESHES:
        verts, faces = MC.mesh(name)[:2]
        grid = MC.host_build(host, verts, faces, G)
        assert grid["tris"][:, 3].all() and MC.lists_of(grid["cell_start"], grid["cell_list"]) == MC.ref_lists(grid["tris"], grid["aabb"], G)
        assert np.array_equal(grid["tris"][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3), verts[faces])
    verts, faces, box, n_bad = bad_mesh()
    grid = MC.host_build(host, verts, faces, G, aabb=box)
    lists = MC.lists_of(grid["cell_start"], grid["cell_list"])
    assert lists == MC.ref_lists(grid["tris"], grid["aabb"], G)
    listed = set(f for v in lists.values() for f in v)
    assert listed == set(range(n_bad, faces.shape[0]))  # every good face somewhere, none of the bad ones
    assert not grid["tris"][:4, 3].any() and grid["tris"][4, 3] == 1  # the face outside the box is VALID, and still absent


def test_invalid_and_outside_faces_are_never_hit(host):
    verts, faces, box, n_bad = bad_mesh()
    good_v, good_f = MC.icosphere()
    o, d, tr = MC.mixed_rays("icosphere")
    extra = (np.array([[2.2, 2.2, 0]], np.float32), np.array([[0, 0, 1]], np.float32), np.array([[0, 4]], np.float32))  # through the outside face
    o, d, tr = (np.concatenate([a, b]) for a, b in zip((o, d, tr), extra))
    want = MC.host_cast(host, MC.host_build(host, good_v, good_f, 1), o, d, tr)
    for G in (1, 5):
        got = MC.host_cast(host, MC.host_build(host, verts, faces, G, aabb=box), o, d, tr)
        assert np.array_equal(got["t"], want["t"]) and np.array_equal(got["face"], np.where(want["face"] >= 0, want["face"] + n_bad, -1))
        assert got["face"][-1] == -1
    # all faces invalid, F = 0, R = 0
    got = MC.host_cast(host, MC.host_build(host, verts, faces[:4], 5, aabb=box), o, d, tr)
    assert (got["face"] == -1).all() and (got["n_tests"] == 0).all() and np.array_equal(got["t"], tr[:, 0])
    empty = MC.host_build(host, good_v, good_f[:0], 5)
    got = MC.host_cast(host, empty, o, d, tr)
    assert (got["face"] == -1).all() and (got["n_tests"] == 0).all() and np.array_equal(got["t"], tr[:, 0]) and not got["u"].any()
    assert all(a.size == 0 for a in MC.host_cast(host, MC.host_build(host, good_v, good_f, 5), o[:0], d[:0], tr[:0]).values())


def test_degenerate_rays(host):
    verts, faces = MC.cube()
    o, d, tr, _ = MC.degenerate_rays()
    for G in (1, 2, 5, 32):
        MC.check_degenerate(MC.host_cast(host, MC.host_build(host, verts, faces, G), o, d, tr))
    t_clip, code = np.full((len(o), 2), 7.0, np.float32), np.full(len(o), 7, np.int32)
    grid = MC.host_build(host, verts, faces, 2)
    host.meshray_host_clip(o.ctypes.data, d.ctypes.data, tr.ctypes.data, grid["aabb"].ctypes.data, len(o), t_clip.ctypes.data, code.ctypes.data)
    assert sorted(set(code.tolist())) == [0, 1, 2] and (t_clip[code == 2, 0] <= t_clip[code == 2, 1]).all()
    # a coplanar duplicate of every face, listed later: the lower index wins every hit
    o, d, tr = MC.mixed_rays("cube")
    want = MC.host_cast(host, MC.host_build(host, verts, faces, 1), o, d, tr)
    for G in (1, 5):
        got = MC.host_cast(host, MC.host_build(host, verts, np.concatenate([faces, faces]), G), o, d, tr)
        assert MC.same_hits(got, want) and (want["face"] >= 0).sum() > 600
        got = MC.host_cast(host, MC.host_build(host, verts, np.concatenate([faces[::-1], faces]), G), o, d, tr)  # the duplicate comes FIRST
        assert np.array_equal(got["t"], want["t"]) and np.array_equal(got["face"][want["face"] >= 0], 11 - want["face"][want["face"] >= 0])
    # refused parameters
    for G in (0, 129, -1):
        MC.host_build(host, verts, faces, G, expect_ok=False)
    grid = MC.host_build(host, verts, faces, 2)
    MC.host_cast(host, dict(grid, G=0), o, d, tr, expect=-1)
    MC.host_cast(host, dict(grid, G=129), o, d, tr, expect=-1)
    MC.host_cast(host, dict(grid, F=-1), o, d, tr, expect=-1)
    # a box without extent: nothing is listed, every ray is rejected
    flat = MC.default_aabb(verts)
    flat[1, 2] = flat[0, 2]
    grid = MC.host_build(host, verts, faces, 2, aabb=flat)
    got = MC.host_cast(host, grid, o, d, tr)
    assert grid["cell_list"].size == 0 and (got["face"] == -1).all() and (got["n_tests"] == 0).all()


def test_clip_rejects_before_it_tests_a_slab(host):
    """csrc/ray_math.hpp's clip_ray, shared with the sphere tracer: every REJECT is decided before the first slab, so a rejected ray that also
    misses the box has code 0, not 1.  On the unit box, each ray with the x axis parallel (d.x == 0) and o.x outside it: a NaN in d.y, a zero
    direction, t0 > t1 -- code 0 --, and a finite non-zero ray -- code 1; t_clip stays (t0, t0).  The tracer's entry lets none of them in."""
    import hashtrace_checks as TC
    o = np.array([[2, 0.5, 0.5]] * 4, np.float32)
    d = np.array([[0, np.nan, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1]], np.float32)
    tr = np.array([[0.25, 4], [0.25, 4], [3, 2], [0.25, 4]], np.float32)
    box = np.array([0, 0, 0, 1, 1, 1], np.float32)
    t_clip, code = np.full((4, 2), 7.0, np.float32), np.full(4, 7, np.int32)
    host.meshray_host_clip(o.ctypes.data, d.ctypes.data, tr.ctypes.data, box.ctypes.data, 4, t_clip.ctypes.data, code.ctypes.data)
    assert code.tolist() == [0, 0, 0, 1] and np.array_equal(t_clip, tr[:, [0, 0]]), (code, t_clip)
    t_clip, ok = TC.host_clip(TC.build_host(), o, d, tr, {"aabb": torch.from_numpy(box.reshape(2, 3))})
    assert not ok.any() and np.array_equal(t_clip, tr[:, [0, 0]]), (ok, t_clip)


def test_twin_runs_clean_under_the_sanitizers():
    """the stand-alone program beside the twin, AddressSanitizer + UndefinedBehaviorSanitizer, run directly with nothing preloaded"""
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(MC.TWIN)), exist_ok=True)
    r = subprocess.run([host_twin.sanitized_main(MC.TWIN)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "meshray_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_kernels_use_no_scratch(tmp_path):
    """csrc/meshray.hip compiled for gfx950 as the build does: no private segment and no spills in any kernel, no LDS in the cast; the figures go
    to profiles/meshray_kernel_resources.txt"""
    kernels = host_twin.kernel_metadata("meshray.hip", tmp_path)
    names = [re.search(r"k_mesh\w+?(?=P|E|$)", k["name"]).group(0) if re.search(r"k_mesh\w+", k["name"]) else k["name"] for k in kernels]
    assert len(kernels) == 7 and any("k_mesh_raycast" in k["name"] for k in kernels), names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "agpr_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
    asm, = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "amdgcn" in f]
    text = open(tmp_path / asm).read()
    lds = [int(x) for x in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", text)]
    occ = [int(x) for x in re.findall(r"^; Occupancy: (\d+)", text, flags=re.M)]
    order = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, flags=re.M)
    assert len(lds) == len(occ) == len(order) == 7, (lds, occ, order)
    by_name = {n: (b, w) for n, b, w in zip(order, lds, occ)}
    cast, = [k for k in kernels if "k_mesh_raycast" in k["name"]]
    assert by_name[cast["name"]][0] == 0 and by_name[cast["name"]][1] >= 4 and cast["vgpr_count"] <= 128, (cast, by_name[cast["name"]])
    lines = ["%s  V %d A %d scratch %d spill %d LDS %d occ %d\n" % (re.sub(r"^_ZN5lab4d\d+|P.*$|E.*$", "", k["name"]), k["vgpr_count"], k["agpr_count"],
                                                                   k["private_segment_fixed_size"], k["vgpr_spill_count"] + k["sgpr_spill_count"],
                                                                   *by_name[k["name"]]) for k in kernels]
    path = os.path.join(host_twin._lib.ROOT, "profiles", "meshray_kernel_resources.txt")
    if not os.path.exists(path) or open(path).read() != "".join(lines):
        with open(path, "w") as fh:
            fh.writelines(lines)


def test_host_layer_checks_its_arguments():
    from lab4d_amd import proxy
    verts, faces = (torch.from_numpy(a) for a in MC.cube())
    o, d, tr = (torch.from_numpy(a) for a in MC.rays("cube", "hit", N_HIT))
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshray.MeshGrid(verts, faces)
    with pytest.raises(RuntimeError, match=r"verts must be float32 \(V, 3\)"):
        meshray.MeshGrid(verts.double(), faces)
    with pytest.raises(RuntimeError, match=r"faces must be int32 \(F, 3\).*convert int64"):
        meshray.MeshGrid(verts, faces.long())
    with pytest.raises(RuntimeError, match="verts must be a device tensor, got ndarray"):
        meshray.MeshGrid(MC.cube()[0], faces)
    for fn, args in ((meshray._check_G, (0,)), (meshray._check_G, (129,)), (meshray._check_G, (2.0,))):
        with pytest.raises(RuntimeError, match=r"outside \[1, 128\]"):
            fn(*args)
    with pytest.raises(RuntimeError, match=r"origin must be float32 \(R, 3\)"):
        meshray._check_rays(o.double(), d, tr)
    with pytest.raises(RuntimeError, match="disagree"):
        meshray._check_rays(o, d, tr[:5])
    with pytest.raises(RuntimeError, match="disagree"):
        meshray._check_rays(o, d[:5], tr)
    with pytest.raises(RuntimeError, match="no CPU path"):
        meshray._check_rays(o, d, tr)
    assert [meshray.default_G(F) for F in (0, 1, 12, 1280, 54668, 10 ** 7)] == [1, 1, 1, 10, 65, 128]
    assert meshray.work_ints(1) == 2 and meshray.work_ints(128) == 128 ** 3 + 2048 and meshray.work_ints(5) == 126
    assert np.array_equal(meshray.default_aabb(verts).numpy(), MC.default_aabb(verts.numpy()))
    flat = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert np.array_equal(meshray.default_aabb(flat).numpy(), MC.default_aabb(flat.numpy())) and float(meshray.default_aabb(flat)[1, 2]) == 2.0 ** -10
    assert callable(proxy.ray_range)
    # Hits.xyz / Hits.normal are plain torch: exact zeros for missed rays, a gradient in verts for the others
    v = verts.clone().requires_grad_(True)
    hits = meshray.Hits(torch.tensor([1.0, 0.0]), torch.tensor([0, -1], dtype=torch.int32), torch.tensor([0.25, 0.0]), torch.tensor([0.5, 0.0]),
                        torch.tensor([1, 0], dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32), torch.tensor([True, False]))
    xyz, n = hits.xyz(v, faces), hits.normal(v, faces)
    a, b, c = verts[faces[0].long()]
    assert torch.allclose(xyz[0], a + 0.25 * (b - a) + 0.5 * (c - a)) and not xyz[1].any() and not n[1].any()
    assert torch.allclose(n[0], torch.tensor([0.0, 0.0, -1.0]))
    g, = torch.autograd.grad(xyz.sum(), v)
    assert torch.allclose(g[faces[0].long()].sum(), torch.tensor(3.0)) and float(g.abs().sum()) == 3.0


def test_c_abi_checks_its_arguments_before_any_launch():
    """the entry points refuse bad arguments with the library's error code and a message; nothing is launched (no GPU here); F = 0 and R = 0 succeed"""
    from lab4d_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(origin=p, dir=p, t_range=p, R=4, tris=p, n_faces=3, aabb=p, G=4, cell_start=p, cell_list=p, t=p, face=p, u=p, v=p, front=p, n_tests=p)

    def cast(**kw):
        a = dict(ok, **kw)
        return lib.lab4d_mesh_raycast(*[a[k] for k in ok], None)

    for kw, msg in [(dict(R=-1), "R = -1"), (dict(G=0), "G = 0 outside [1, 128]"), (dict(G=129), "G = 129"), (dict(n_faces=-1), "n_faces = -1"),
                    (dict(n_faces=2 ** 31 // 12 + 1), "n_faces"), (dict(aabb=None), "null pointer (aabb"), (dict(tris=None), "null pointer (tris"),
                    (dict(cell_start=None), "null pointer (tris"), (dict(origin=None), "null pointer (origin"), (dict(t_range=None), "null pointer (origin"),
                    (dict(t=None), "null pointer (t,"), (dict(n_tests=None), "null pointer (t,")]:
        assert cast(**kw) == -1, kw
        assert msg in lib.lab4d_last_error().decode(), (msg, lib.lab4d_last_error().decode())
    assert cast(R=0) == 0 and cast(R=0, origin=None, dir=None, t_range=None, t=None, face=None, u=None, v=None, front=None, n_tests=None) == 0
    assert cast(R=0, n_faces=0, tris=None, cell_start=None, cell_list=None) == 0 and cast(R=0, aabb=None) == -1
    count = lambda **kw: lib.lab4d_meshgrid_count(*[dict(dict(verts=p, faces=p, n_verts=3, n_faces=1, aabb=p, G=4, tris=p, cell_start=p, work=p, total=p), **kw)[k]  # noqa: E731
                                                    for k in ("verts", "faces", "n_verts", "n_faces", "aabb", "G", "tris", "cell_start", "work", "total")], None)
    for kw, msg in [(dict(G=0), "G = 0"), (dict(G=200), "G = 200"), (dict(n_faces=-2), "n_faces = -2"), (dict(n_verts=-1), "n_verts = -1"),
                    (dict(faces=None), "null pointer (faces"), (dict(tris=None), "null pointer (faces"), (dict(verts=None), "null pointer (verts)"),
                    (dict(work=None), "null pointer (cell_start"), (dict(total=None), "null pointer (cell_start")]:
        assert count(**kw) == -1, kw
        assert msg in lib.lab4d_last_error().decode(), (msg, lib.lab4d_last_error().decode())
    assert count(n_faces=0) == 0 and count(n_faces=0, verts=None, faces=None, tris=None, cell_start=None, work=None, total=None) == 0
    fill = lambda **kw: lib.lab4d_meshgrid_fill(*[dict(dict(tris=p, n_faces=1, aabb=p, G=4, cell_start=p, work=p, n_list=2, cell_list=p), **kw)[k]  # noqa: E731
                                                  for k in ("tris", "n_faces", "aabb", "G", "cell_start", "work", "n_list", "cell_list")], None)
    for kw, msg in [(dict(G=0), "G = 0"), (dict(n_list=-1), "n_list = -1"), (dict(n_faces=-1), "n_faces = -1"), (dict(cell_list=None), "null pointer (tris")]:
        assert fill(**kw) == -1, kw
        assert msg in lib.lab4d_last_error().decode(), (msg, lib.lab4d_last_error().decode())
    assert fill(n_faces=0) == 0 and fill(n_list=0, cell_list=None) == 0
    assert lib.lab4d_meshgrid_pack(p, p, 3, -1, p, None) == -1 and lib.lab4d_meshgrid_pack(p, None, 3, 1, p, None) == -1
    assert lib.lab4d_meshgrid_pack(None, None, 0, 0, None, None) == 0
    assert _lib.SIGNATURES["lab4d_mesh_raycast"][1][3] is ctypes.c_long and all(_lib.SIGNATURES[n][2] for n in _lib.SIGNATURES if "mesh_raycast" in n or "meshgrid" in n)
