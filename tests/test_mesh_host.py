"""The iso-surface extractor on the CPU: the generated case table (tools/gen_mc_tables.py -> lab4d_amd/csrc/mc_tables.hpp) and the CPU twin
of the kernels (tests/host_harness/mesh_host.cpp: the same csrc/mesh_math.hpp functions, the same table, the ordering contract of
include/lab4d_mesh.h).  There is no skimage to compare with: the mesh is pinned by the properties of tests/mesh_checks.py.  The GPU suite
(tests/test_gpu_zzzmesh.py) then holds the kernels bit for bit to this twin.  CPU only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import mesh_checks as MC  # noqa: E402

ROOT = MC.ROOT


@pytest.fixture(scope="module")
def host():
    return MC.build_host()


@pytest.fixture(scope="module")
def gen():
    return MC.gen_module()


@pytest.fixture(scope="module")
def tri_count(gen):
    return np.array([len(t) for t in gen.table()])


def test_committed_table_is_what_the_generator_writes(tmp_path):
    out = tmp_path / "mc_tables.hpp"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_mc_tables.py"), "--out", str(out)])
    assert out.read_bytes() == open(os.path.join(ROOT, "lab4d_amd", "csrc", "mc_tables.hpp"), "rb").read()


def test_every_case_of_the_table_is_a_consistent_patch(gen):
    tab = gen.table()
    assert len(tab) == 256 and max(len(t) for t in tab) == 5 and sum(len(t) for t in tab) == 820
    for case, tris in enumerate(tab):
        inside = [(case >> c) & 1 for c in range(8)]
        crossed = {n for n, (a, b) in enumerate(gen.EDGES) if inside[a] != inside[b]}
        assert {e for t in tris for e in t} == crossed, case
        assert len(tris) <= 5
        directed = [(t[m], t[(m + 1) % 3]) for t in tris for m in range(3)]
        assert len(set(directed)) == len(directed), case  # no directed edge twice
        for a, b in directed:
            interior = (b, a) in directed
            # a matched edge is interior to the patch and must not lie in a cell face (it would coincide with the neighbour's segment);
            # an unmatched one is the patch boundary and must lie in a cell face (the neighbour cell supplies its reverse)
            assert gen.in_one_face(a, b) != interior, (case, a, b)


@pytest.mark.parametrize("shape,seed", [((14, 14, 14), 5), ((9, 12, 17), 1)])
def test_random_volume_is_closed_manifold_and_in_contract_order(host, tri_count, shape, seed):
    vol = MC.random_volume(shape, seed)
    v, f = MC.host_extract(host, vol)
    MC.assert_closed(v, f)
    n_crossed = sum(int(((vol < 0).take(range(0, shape[a] - 1), a) != (vol < 0).take(range(1, shape[a]), a)).sum()) for a in range(3))
    assert v.shape[0] == n_crossed
    MC.assert_matches_contract(v, f, vol, None, 0.0, tri_count)
    if shape == (14, 14, 14):  # (the seed is chosen so that) all 256 sign configurations are exercised
        assert np.unique(MC.cell_cases(vol, 0.0)).size == 256


def test_sphere_torus_and_two_spheres(host, tri_count):
    G = 32
    origin, step = MC.world(G)
    sph = MC.sphere(G, 0.3)
    v, f = MC.host_extract(host, sph, origin=origin, step=step)
    MC.assert_closed(v, f)
    assert MC.euler(v, f) == 2 and MC.signed_volume(v, f) > 0
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.3).max()
    assert err <= MC.sphere_bound(G, 0.3), (err, MC.sphere_bound(G, 0.3))
    vi, fi = MC.host_extract(host, sph)
    assert np.array_equal(fi, f)
    MC.assert_matches_contract(vi, fi, sph, None, 0.0, tri_count)
    assert np.abs(v - (vi * step + origin)).max() <= 2 * np.spacing(np.float32(0.5))

    v, f = MC.host_extract(host, MC.torus(G), origin=origin, step=step)
    MC.assert_closed(v, f)
    assert MC.euler(v, f) == 0 and MC.signed_volume(v, f) > 0

    v, f = MC.host_extract(host, MC.two_spheres(G), origin=origin, step=step)
    MC.assert_closed(v, f)
    assert MC.euler(v, f) == 4
    lv, lf = MC.host_largest_component(host, v, f)
    big = v[:, 0] < 0.04  # (the two spheres are separated by x in [-0.07, 0.15])
    assert 0 < big.sum() < v.shape[0] and big.sum() > (~big).sum()
    assert np.array_equal(lv, v[big])  # exactly the larger sphere's vertices, in their original order
    MC.assert_closed(lv, lf)
    assert MC.euler(lv, lf) == 2 and MC.signed_volume(lv, lf) > 0
    assert np.array_equal(lv[lf], v[f[big[f[:, 0]]]])  # the surviving faces, re-indexed, in their original order


def test_component_tie_goes_to_the_smallest_vertex_index(host):
    G = 32
    origin, step = MC.world(G)
    v, f = MC.host_extract(host, MC.three_blobs(G), origin=origin, step=step)
    MC.assert_closed(v, f)
    assert MC.euler(v, f) == 6
    left, right = (v[:, 0] < -0.1), (v[:, 0] > 0.1)
    assert left.sum() == right.sum() > (~(left | right)).sum() > 0  # a genuine tie between the two largest
    lv, lf = MC.host_largest_component(host, v, f)
    assert np.array_equal(lv, v[left])
    MC.assert_closed(lv, lf)


def test_mask_and_nan_skip_cells(host, tri_count):
    G = 32
    sph = MC.sphere(G, 0.3)
    X, _, _ = MC.grid_xyz(G)
    mask = (X < 0.05)
    v, f = MC.host_extract(host, sph, mask=mask)
    assert f.shape[0] > 0
    MC.assert_matches_contract(v, f, sph, mask, 0.0, tri_count)  # (face count == triangles of the MESHED cells only, each face inside its cell)
    assert np.array_equal(np.unique(f), np.arange(v.shape[0]))  # every vertex is referenced
    live = MC.meshed_cells(sph, mask)
    cells = MC.expected_face_cells(sph, mask, 0.0, tri_count)
    assert live[cells[:, 0], cells[:, 1], cells[:, 2]].all()
    # every open edge lies in a cell face whose other side is a skipped cell
    rows, dup = MC.unpaired_edges(f, v.shape[0])
    assert dup == 0 and rows.size > 0
    e = MC.directed_edges(f)[rows]
    owner = cells[rows % f.shape[0]]
    for (a, b), c in zip(e, owner):
        ok = False
        for d in range(3):
            if v[a, d] == v[b, d] and v[a, d] in (c[d], c[d] + 1):
                n = c.copy()
                n[d] += 1 if v[a, d] == c[d] + 1 else -1
                ok = ok or not (0 <= n[d] < G - 1) or not live[n[0], n[1], n[2]]
        assert ok, (a, b, c)

    bad = sph.copy()
    p = (16, 16, 25)  # next to the surface (|p| - 0.3 changes sign between k = 24 and 25 on this axis)
    assert sph[16, 16, 24] < 0 < sph[16, 16, 26]
    bad[p] = np.nan
    v, f = MC.host_extract(host, bad)
    assert np.isfinite(v).all() and f.shape[0] > 0
    MC.assert_matches_contract(v, f, bad, None, 0.0, tri_count)
    cell = np.floor(v[f].mean(1)).astype(int)  # (centroid of a triangle whose corners lie on the cell's edges)
    around = np.all((cell >= np.array(p) - 1) & (cell <= np.array(p)), 1)
    assert not around.any()
    v_inf, f_inf = MC.host_extract(host, np.where(np.isnan(bad), np.float32(np.inf), bad))
    assert np.array_equal(v_inf, v) and np.array_equal(f_inf, f)


def test_level_moves_the_surface(host):
    G = 32
    origin, step = MC.world(G)
    v, f = MC.host_extract(host, MC.sphere(G, 0.3), level=0.005, origin=origin, step=step)
    MC.assert_closed(v, f)
    assert MC.euler(v, f) == 2
    err = np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.305).max()
    assert err <= MC.sphere_bound(G, 0.3), (err, MC.sphere_bound(G, 0.3))


def test_empty_and_full_volumes_give_nothing(host):
    for vol in (np.ones((7, 8, 9), np.float32), -np.ones((7, 8, 9), np.float32), np.ones((1, 1, 1), np.float32), np.ones((5, 1, 4), np.float32)):
        v, f = MC.host_extract(host, vol)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_mesh_entry_points_validate_before_any_launch():
    """include/lab4d_mesh.h through ctypes, without a GPU: null volume, zero dimension, too large a grid -> LAB4D_EINVAL and a message."""
    from lab4d_amd import _lib
    _lib.build(verbose=False)
    so = _lib.lib()  # (the signatures: from include/lab4d_mesh.h)
    buf = ctypes.create_string_buffer(64)
    b = ctypes.cast(buf, ctypes.c_void_p)
    assert so.lab4d_mesh_count(None, None, 4, 4, 4, 0.0, b, b, None) == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_mesh_count(b, None, 4, 0, 4, 0.0, b, b, None) == -1 and b">= 1" in so.lab4d_last_error()
    assert so.lab4d_mesh_count(b, None, 1024, 1024, 1024, 0.0, b, b, None) == -1 and b"too large" in so.lab4d_last_error()
    assert so.lab4d_mesh_count(b, None, 4, 4, 4, float("nan"), b, b, None) == -1 and b"NaN" in so.lab4d_last_error()
    assert so.lab4d_mesh_emit(None, 4, 4, 4, 0.0, None, b, 1, 1, b, b, None) == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_mesh_emit(b, 4, 4, -1, 0.0, None, b, 1, 1, b, b, None) == -1
    assert so.lab4d_mesh_emit(b, 4, 4, 4, 0.0, None, b, -1, 1, b, b, None) == -1 and b"negative" in so.lab4d_last_error()
    assert so.lab4d_mesh_emit(b, 4, 4, 4, 0.0, None, b, 1, 1, None, b, None) == -1 and b"null output" in so.lab4d_last_error()
    assert so.lab4d_mesh_emit(b, 4, 4, 4, 0.0, None, b, 4 * 4 * 4 * 3 + 1, 1, b, b, None) == -1 and b"exceed" in so.lab4d_last_error()
    assert so.lab4d_mesh_largest_component(b, b, -1, 0, b, b, b, b, None, None) == -1
    assert so.lab4d_mesh_largest_component(None, b, 3, 1, b, b, b, b, None, None) == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_mesh_work_ints(0, 4, 4) == -1 and so.lab4d_mesh_work_ints(1024, 1024, 1024) == -1
    n = 5 * 6 * 7
    assert so.lab4d_mesh_work_ints(5, 6, 7) == 3 * n + 2 * ((n + 3) // 4) + 2 * ((n + 255) // 256)
    assert so.lab4d_mesh_component_work_ints(-1, 0) == -1 and so.lab4d_mesh_component_work_ints(10, 20) >= 30


def test_mesh_refuses_cpu_tensors():
    import torch
    from lab4d_amd import mesh
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.marching_cubes(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.keep_largest_component(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))


def test_mesh_object_has_the_fields_the_bound_updates_read():
    from lab4d_amd import mesh
    m = mesh.Mesh(np.array([[0, 1, 2], [3, -1, 5], [1, 1, 1]], np.float64), np.array([[0, 1, 2]]))
    assert m.vertices.dtype == np.float32 and m.faces.dtype == np.int32 and m.faces.shape == (1, 3)
    assert np.array_equal(m.bounds, np.array([[0, -1, 1], [3, 1, 5]], np.float32))
    assert mesh.Mesh(np.zeros((0, 3)), np.zeros((0, 3))).bounds is None


def test_no_mesh_kernel_uses_scratch(tmp_path):
    """csrc/mesh.hip compiled for gfx950 as the build does: every kernel's code-object metadata reports no private segment and no spills."""
    kernels = host_twin.kernel_metadata("mesh.hip", tmp_path)
    names = [k["name"] for k in kernels]
    assert len(names) >= 14 and all(n.startswith("_ZN5lab4d") and ("k_mc_" in n or "k_cc_" in n) for n in names), names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
