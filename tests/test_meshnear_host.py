"""The grid distance query's CPU twin (tests/host_harness/meshnear/meshnear_host.cpp over lab4d_amd/csrc/meshnear_math.hpp), no GPU: the walk at
G = 2, 5, 32 against G = 1 and G = 1 against the brute-force twin word for word (the test of the stop rule and its margin), the restated
closest-point function against lab4d_msdf::closest_d2, the pseudonormal sign against the analytic cube, float64 winding and the rule restated
in float64, the edge cases, the stand-alone program under the sanitizers, the kernel's code-object metadata and the Python layer's guards."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import meshnear_checks as NC  # noqa: E402
import meshray_checks as MC  # noqa: E402
import meshsdf_checks as SD  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def twin(verts, faces, pts, G, sign_mode=1, orient=1, aabb=None):
    return NC.host_closest(NC.build_host(), MC.host_build(MC.build_host(), verts, faces, G, aabb=aabb), pts, sign_mode, orient)


@pytest.mark.parametrize("name", MC.MESHES)
def test_every_G_equals_G1_equals_brute_force(name):
    """d2, face, closest, region at G = 2, 5, 32 == G = 1 word for word; G = 1 == meshsdf_host.cpp in |sdf|, d2, face and closest word for word, on
    EVERY point of the set (inside, 1 / 8 / 1,024 extents outside, on every vertex, edge midpoint and centroid, on cell walls and grid corners):
    nothing is left out.  n_tests at G = 1 is the number of valid faces."""
    verts, faces = MC.mesh(name)[:2]
    pts, where = NC.points(name)
    ref = twin(verts, faces, pts, 1)
    NC.check_outputs_sane(ref, faces.shape[0])
    assert (ref["n_tests"] == faces.shape[0]).all() and (ref["face"] >= 0).all()
    assert set(np.unique(ref["region"])) == set(range(7))
    for G in (2, 5, 32):
        got = twin(verts, faces, pts, G)
        bad = [int((bits(got[k]) != bits(ref[k])).sum()) for k in ("d2", "face", "closest", "region", "sdf")]
        print("%s G = %d: mean n_tests %.1f (max %d), mean cells %.1f; words that differ from G = 1: %s"
              % (name, G, got["n_tests"].mean(), got["n_tests"].max(), got["n_cells"].mean(), bad))
        assert NC.same_words(got, ref) and np.array_equal(bits(got["sdf"]), bits(ref["sdf"])), (G, bad)
    brute = SD.host_query(SD.build_host(), verts, faces, pts)
    # (no mask anywhere: the comparisons below run on every point of the set, so the share left out is 0)
    assert np.array_equal(bits(np.abs(ref["sdf"])), bits(np.abs(brute["sdf"]))) and np.array_equal(bits(ref["d2"]), bits(brute["d2"]))
    assert np.array_equal(ref["face"], brute["face"]) and np.array_equal(bits(ref["closest"]), bits(brute["closest"]))
    unsigned = twin(verts, faces, pts, 5, sign_mode=0)
    assert NC.same_words(unsigned, ref) and np.array_equal(bits(unsigned["sdf"]), bits(np.abs(ref["sdf"])))


def region64(p, t):
    """Ericson's classification in float64 on (n, 3) points and (n, 3, 3) triangles: region (n,) and margin (n,): the smallest normalised distance
    of a quantity the cascade compares from its threshold"""
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
             (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    codes = [4, 5, 1, 6, 2, 3]
    region = np.zeros(p.shape[0], int)
    for cond, code in list(zip(conds, codes))[::-1]:
        region = np.where(cond, code, region)
    edge = np.maximum(np.linalg.norm(ab, axis=1), np.maximum(np.linalg.norm(ac, axis=1), np.linalg.norm(c - b, axis=1)))
    reach = np.maximum(np.linalg.norm(ap, axis=1), np.maximum(np.linalg.norm(bp, axis=1), np.linalg.norm(cp, axis=1)))
    lin = np.abs(np.stack([d1, d2, d3, d4, d5, d6, d4 - d3, d5 - d6], 1)) / (edge * reach)[:, None]
    quad = np.abs(np.stack([va, vb, vc], 1)) / ((edge * reach) ** 2)[:, None]
    return region, np.minimum(lin.min(1), quad.min(1))


def test_restated_closest_point_is_bit_equal_and_names_the_region():
    """closest_reg == lab4d_msdf::closest_d2 bit for bit in d2 and q on 10^5 random (point, triangle) pairs; its region is float64's wherever
    float64's margins to the region boundaries exceed 1e-5 relative; every region occurs among those"""
    rng = np.random.default_rng(11)
    n = 100000
    tri = rng.random((n, 9)).astype(np.float32)
    pts = (rng.random((n, 3)) * 3 - 1).astype(np.float32)
    pts[:n // 4] = (tri[:n // 4].reshape(-1, 3, 3) * rng.dirichlet(np.ones(3), n // 4)[:, :, None]).sum(1) + rng.normal(0, 0.05, (n // 4, 3))  # near the face
    new, old, region = np.full((n, 4), 7, np.float32), np.full((n, 4), 8, np.float32), np.full(n, -7, np.int32)
    NC.build_host().meshnear_host_restated(pts.ctypes.data, tri.ctypes.data, n, new.ctypes.data, region.ctypes.data, old.ctypes.data)
    assert np.array_equal(bits(new), bits(old))
    r64, margin = region64(pts.astype(np.float64), tri.astype(np.float64).reshape(n, 3, 3))
    safe = margin > 1e-5
    print("restated: %d of %d pairs with a float64 margin above 1e-5; regions among them %s" % (safe.sum(), n, np.bincount(r64[safe], minlength=7)))
    assert safe.mean() > 0.9 and (np.bincount(r64[safe], minlength=7) > 500).all()
    assert np.array_equal(region[safe], r64[safe])


def chosen_points(name, verts, faces, pts, ref):
    """the points whose sign is compared: float64 distance above 1e-5 L (L: the box diagonal); and the float64 brute-force reference"""
    r64 = SD.ref_query(verts, faces, pts)
    L = float(np.linalg.norm(np.diff(MC.default_aabb(verts).astype(np.float64), axis=0)))
    return np.sqrt(r64["d2"]) > NC.OFF_SURFACE * L, r64, L


@pytest.mark.parametrize("name", ("cube", "icosphere"))
def test_sign_on_closed_meshes_in_both_orientations(name):
    """orient = the numpy restatement of "auto": inside / outside == the analytic cube, == float64 winding on the icosphere, at every point farther
    than 1e-5 L from the surface, mesh as given and with every face flipped; on-surface points: d within 7e's bound of 0 and a finite sdf.  A
    fixed orient = +1 on the inward-oriented mesh flips every sign.  No chosen point has |s| <= 1e-4 |p - q| |n| in float64 (asserted: a
    condition on the inputs), which leaves the device's own atan2f no room to change a sign."""
    verts, faces = MC.mesh(name)[:2]
    pts, where = NC.points(name)
    for flip in (False, True):
        fc = SD.flipped(faces) if flip else faces
        orient = NC.volume_orient(verts, fc)
        assert orient == (-1 if flip else 1)
        got = twin(verts, fc, pts, 5, orient=orient)
        chosen, r64, L = chosen_points(name, verts, fc, pts, got)
        inside = ((pts > MC.CUBE_LO) & (pts < MC.CUBE_HI)).all(1) if name == "cube" else np.abs(r64["w"]) > 0.5
        assert chosen.sum() > 400 and inside[chosen].sum() > 50
        assert np.array_equal(got["sdf"][chosen] < 0, inside[chosen]), np.nonzero((got["sdf"] < 0) != inside)[0][:10]
        on = ~chosen
        assert np.isfinite(got["sdf"][on]).all() and (got["d2"][on].astype(np.float64) <= r64["d2"][on] + SD.d2_bound(SD.bbox_diagonal(verts, pts[on]))).all()
        for k in ("verts", "edges", "faces"):
            assert (np.abs(got["sdf"][where[k]]) <= np.sqrt(SD.d2_bound(L))).all()
        s, scale, n_inc = NC.ref_side(verts, fc, pts, got)
        assert (np.abs(s[chosen]) > NC.S_MARGIN * scale[chosen]).all(), np.nonzero(chosen & (np.abs(s) <= NC.S_MARGIN * scale))[0][:10]
        assert np.array_equal(orient * s[chosen] < 0, got["sdf"][chosen] < 0)
        assert (n_inc[(got["region"] >= 1) & (got["region"] <= 3)] == 2).all() and (n_inc[got["region"] >= 4] >= 4).all()  # closed and welded
        if flip:
            fixed = twin(verts, fc, pts, 5, orient=1)
            assert np.array_equal(fixed["sdf"][chosen] < 0, ~inside[chosen]) and NC.same_words(fixed, got)


def test_every_voronoi_region_of_the_cube():
    """points built over a face's interior, an edge's interior and a corner, 1 / 8 outside (all three kinds) and 1 / 8 inside (the face; inside a
    convex body the closest feature is always a face): the expected region kind, the exact distance and the exact sign"""
    verts, faces = MC.cube()
    lo, hi = MC.CUBE_LO, MC.CUBE_HI
    rows = []  # (point, kind, signed distance)
    for axis in range(3):
        for side in (0, 1):
            wall = (hi if side else lo)[axis]
            out = 1 if side else -1
            p = lo + np.array([0.25, 0.625, 0.375]) * (hi - lo)  # off the diagonals of the sides
            for d in (0.125, -0.125):
                q = p.copy()
                q[axis] = wall + out * d
                rows.append((q, "face", d))
            for axis2 in range(axis + 1, 3):
                for side2 in (0, 1):
                    q = p.copy()
                    q[axis], q[axis2] = wall + out * 0.125, (hi if side2 else lo)[axis2] + (1 if side2 else -1) * 0.125
                    rows.append((q, "edge", 0.125 * 2 ** 0.5))
    for corner in range(8):
        sel = np.array([(corner >> a) & 1 for a in range(3)])
        rows.append((np.where(sel, hi + 0.125, lo - 0.125), "vertex", 0.125 * 3 ** 0.5))
    pts = np.array([r[0] for r in rows], np.float32)
    for G in NC.SIZES_G:
        got = twin(verts, faces, pts, G)
        for i, (_, kind, d) in enumerate(rows):
            reg = int(got["region"][i])
            assert {"face": reg == 0, "edge": 1 <= reg <= 3, "vertex": reg >= 4}[kind], (G, i, kind, reg)
            assert got["sdf"][i] == np.float32(d), (G, i, kind, got["sdf"][i], d)
    assert sum(r[1] == "face" for r in rows) == 12 and sum(r[1] == "edge" for r in rows) == 12 and sum(r[1] == "vertex" for r in rows) == 8


def test_open_hemisphere_takes_the_side_of_the_nearest_feature():
    """the sign equals the rule restated in numpy float64 on every chosen point, none of them within the margin; below the rim the answer is the
    side of the rim's face, edge or vertex: points straight below a rim feature are 'inside' the open shell although the winding number says
    outside"""
    verts, faces = MC.mesh("hemisphere")[:2]
    pts, where = NC.points("hemisphere")
    got = twin(verts, faces, pts, 5)
    chosen, r64, L = chosen_points("hemisphere", verts, faces, pts, got)
    s, scale, n_inc = NC.ref_side(verts, faces, pts, got)
    assert (np.abs(s[chosen]) > NC.S_MARGIN * scale[chosen]).all(), np.nonzero(chosen & (np.abs(s) <= NC.S_MARGIN * scale))[0][:10]
    assert np.array_equal(s[chosen] < 0, got["sdf"][chosen] < 0)
    rim = (n_inc == 1) & (got["region"] >= 1) & (got["region"] <= 3) & chosen  # an edge with one face: the rim
    assert rim.sum() > 20
    tri = verts.astype(np.float64)[faces[got["face"][rim]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    side = ((pts[rim].astype(np.float64) - got["closest"][rim]) * n).sum(-1)
    assert np.array_equal(side < 0, got["sdf"][rim] < 0)
    differs = (got["sdf"] < 0) != (np.abs(r64["w"]) > 0.5)
    print("hemisphere: %d rim points; the pseudonormal's side differs from |w| > 0.5 on %d of %d chosen points" % (rim.sum(), (differs & chosen).sum(), chosen.sum()))
    assert (differs & chosen).any()


def test_edge_cases():
    verts, faces = MC.cube()
    pts, _ = NC.points("cube")
    ref = twin(verts, faces, pts, 5)
    nan, inf = np.nan, np.inf
    odd = np.array([[nan, 0, 0], [0, nan, 0], [0, 0, nan], [inf, 0, 0], [0, -inf, 0], [0, 0, inf]], np.float32)
    for G in NC.SIZES_G:
        got = twin(verts, faces, odd, G)
        assert np.isnan(got["sdf"]).all() and np.isnan(got["d2"]).all() and (got["face"] == -1).all() and (got["region"] == -1).all()
        assert np.array_equal(bits(got["closest"]), bits(odd)) and (got["n_tests"] == 0).all()
    assert twin(verts, faces, pts[:0], 5)["sdf"].size == 0  # N = 0
    for f_none in (faces[:0], np.array([[0, 1, 99], [5, 5, 6]], np.int32)):  # F = 0; all faces invalid
        got = twin(verts, f_none, pts, 5, aabb=MC.default_aabb(verts))
        assert np.isposinf(got["sdf"]).all() and np.isposinf(got["d2"]).all() and (got["face"] == -1).all() and np.array_equal(bits(got["closest"]), bits(pts))
    bv, bf, box, n_bad = NC.bad_cube()
    for G in (1, 5):
        got = twin(bv, bf, pts, G, aabb=box)  # invalid faces mixed in: never winners, never incident
        assert (got["face"] >= n_bad).all() and np.array_equal(got["face"] - n_bad, ref["face"])
        assert all(np.array_equal(bits(got[k]), bits(ref[k])) for k in ("sdf", "d2", "closest", "region"))
    for first in (faces, np.ascontiguousarray(faces[::-1])):  # coplanar duplicates: the lower index wins, in either order
        alone, got = twin(verts, first, pts, 5), twin(verts, np.concatenate([first, faces]), pts, 5)
        assert (got["face"] < 12).all() and NC.same_words(got, alone) and np.array_equal(bits(got["sdf"]), bits(ref["sdf"]))
    soup = verts[faces].reshape(-1, 3)  # unwelded: 36 vertices, the same coordinates
    got = twin(soup, np.arange(36, dtype=np.int32).reshape(12, 3), pts, 5)
    assert np.array_equal(bits(got["sdf"]), bits(ref["sdf"])) and NC.same_words(got, ref)
    lib, grid = NC.build_host(), MC.host_build(MC.build_host(), verts, faces, 2)
    for G, sign_mode, orient in ((0, 1, 1), (129, 1, 1), (2, 2, 1), (2, -1, 1), (2, 1, 0), (2, 1, 2)):
        NC.host_closest(lib, dict(grid, G=G), pts[:4], sign_mode, orient, expect=-1)
    p4, out = pts[:4].copy(), np.zeros(4, np.float32)
    args = [p4.ctypes.data, 4, grid["tris_buf"].ctypes.data, 12, grid["aabb"].ctypes.data, 2, grid["cell_start"].ctypes.data, grid["cell_list"].ctypes.data, 1, 1,
            out.ctypes.data, None, None, None, None, None, None]
    assert lib.meshnear_host_closest(*args) == 0  # every optional output NULL
    for null_at in (0, 2, 4, 6, 10):  # pts, tris, aabb, cell_start, sdf
        assert lib.meshnear_host_closest(*[None if i == null_at else a for i, a in enumerate(args)]) == -1, null_at


def test_standalone_program_under_the_sanitizers():
    os.makedirs(os.path.join(host_twin.BUILD, "meshnear"), exist_ok=True)
    r = subprocess.run([host_twin.sanitized_main(NC.TWIN)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "meshnear_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_kernel_uses_no_scratch(tmp_path):
    """csrc/meshnear.hip compiled for gfx950 as the build does: no private segment, no spills, no AGPRs, no LDS; the figures go to
    profiles/meshnear_kernel_resources.txt"""
    kernel, = host_twin.kernel_metadata("meshnear.hip", tmp_path)
    assert "k_mesh_closest" in kernel["name"]
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "agpr_count"):
        assert kernel[key] == 0, (key, kernel)
    asm, = [f for f in os.listdir(tmp_path) if f.endswith(".s") and "amdgcn" in f]
    text = open(tmp_path / asm).read()
    lds, = [int(x) for x in re.findall(r"\.amdhsa_group_segment_fixed_size (\d+)", text)]
    occ, = [int(x) for x in re.findall(r"^; Occupancy: (\d+)", text, flags=re.M)]
    assert lds == 0 and occ >= 4 and kernel["vgpr_count"] <= 128, (lds, occ, kernel)
    line = "k_mesh_closest  V %d A %d scratch %d spill %d LDS %d occ %d\n" % (kernel["vgpr_count"], kernel["agpr_count"], kernel["private_segment_fixed_size"],
                                                                             kernel["vgpr_spill_count"] + kernel["sgpr_spill_count"], lds, occ)
    path = os.path.join(host_twin._lib.ROOT, "profiles", "meshnear_kernel_resources.txt")
    if not os.path.exists(path) or open(path).read() != line:
        try:
            with open(path, "w") as fh:
                fh.write(line)
        except OSError:
            pass  # (a read-only checkout: the figures were asserted above)


def test_python_layer_refuses_before_any_launch():
    """argument errors of MeshGrid.closest and of the consumers' grid keyword need no device: they are raised before anything is launched (the
    coverage and capture guards need a grid, hence a device: tests/test_gpu_zzzzzzzzzzzzmeshnear.py)"""
    import torch
    from lab4d_amd import meshray, meshsdf
    g = object.__new__(meshray.MeshGrid)  # no device: the checks come before any use of the grid's buffers
    with pytest.raises(RuntimeError, match="pts must be a device tensor"):
        g.closest(np.zeros((4, 3), np.float32))
    with pytest.raises(RuntimeError, match=r"pts must be float32 \(\.\.\., 3\)"):
        g.closest(torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match=r"pts must be float32 \(\.\.\., 3\)"):
        g.closest(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="sign = 'winding' is neither"):
        g.closest(torch.zeros(4, 3), sign="winding")
    for bad in (0, 2, True, 1.0, "out"):
        with pytest.raises(RuntimeError, match="is not 'auto', \\+1 or -1"):
            g.closest(torch.zeros(4, 3), orient=bad)
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.closest(torch.zeros(4, 3))
    assert meshray.Nearest._fields == ("sdf", "d2", "face", "closest", "region", "n_tests")
    import inspect
    assert inspect.signature(meshsdf.signed_distance).parameters["grid"].default is None
    from lab4d_amd import occgrid, proxy
    assert inspect.signature(proxy.init_sdf_fn).parameters["grid"].default is False
    assert inspect.signature(occgrid.OccupancyGrid.seed_from_mesh).parameters["grid"].default is None
    from lab4d_amd import _lib
    assert _lib.SIGNATURES["lab4d_mesh_closest"][2] and len(_lib.SIGNATURES["lab4d_mesh_closest"][1]) == 17
