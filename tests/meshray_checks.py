"""Shared by tests/test_meshray_host.py (CPU twin against float64) and tests/test_gpu_zzzzzzzzzzzmeshray.py (kernels against the twin): the host
harness of the mesh ray caster (tests/host_harness/meshray/meshray_host.cpp over lab4d_amd/csrc/meshray_math.hpp), the test meshes, the ray
sets and the truth: numpy float64 Moeller-Trumbore over all faces, smallest t.  Nothing of the code under test enters the truth.  Everything
built here is cached and shared between the two suites: never modified.

MESHES  a cube (12 faces, dyadic corners), an icosphere (1,280 faces, r = 0.3) and its open upper hemisphere, as tests/meshsdf_checks.py has them
        (restated).  Each has a centre, a radius r_in of a ball inside the surface and a radius r_out of a ball that holds it.
RAYS    HIT: from 3 r_out off the centre, aimed at a point within 0.8 r_in of it, |d| in 0.5 .. 2.  MISS: the same origins, impact parameter
        >= 1.3 r_out.  INSIDE: origins within 0.5 r_in of the centre.  The sets are CHOSEN with no impact parameter in (0.8 r_in, 1.3 r_out): no
        ray grazes the silhouette of a closed mesh, and the comparisons leave out none."""
import functools
import os

import numpy as np

import host_twin

TWIN = "meshray/meshray"  # tests/host_harness/meshray/meshray_host.cpp: a folder of its own (tests/test_host_twin.py pins the census of the twins beside it)
PAD = np.float32(2.0 ** -10)
# |t - t64| * len, twin against float64: 4 x the largest deviation measured on the HIT, MISS and INSIDE sets of the three meshes at G = 5
# (4.85e-7 on the cube, whose rays are the longest: origins 2.6 off the centre; the icosphere 1.13e-7, the hemisphere 2.01e-7): see DESIGN.md 7j.  4 x and
# not 2 x: the kernel is held to the twin bit for bit, so the margin only has to cover another libm or compiler on the host.
T_BOUND = 1.94e-6
SIZES_R = (1, 63, 64, 65, 1025)


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


# ---------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------
CUBE_LO, CUBE_HI = np.array([-0.5, -0.25, -0.75]), np.array([0.5, 0.75, 0.25])  # dyadic corners: the constructed rays are exact


def cube():
    """12 triangles, outward; faces 2k and 2k + 1 share the diagonal of one side"""
    c = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64)
    verts = (CUBE_LO + c * (CUBE_HI - CUBE_LO)).astype(np.float32)
    faces = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [3, 7, 6], [3, 6, 2], [0, 4, 7], [0, 7, 3], [1, 2, 6], [1, 6, 5]], np.int32)
    return verts, faces


@functools.lru_cache(None)
def icosphere(level=3, r=0.3):
    """20 * 4^level faces (1,280 at level 3), vertices on the sphere of radius r, outward"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
         (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * r).astype(np.float32), np.array(f, np.int32)


def hemisphere(level=3, r=0.3):
    """the faces of the icosphere whose centroid has z > 0: open, with a ragged rim"""
    v, f = icosphere(level, r)
    return v, np.ascontiguousarray(f[v[f].mean(1)[:, 2] > 0])


def sagitta(verts, faces, r):
    """how far the flat faces dip below the sphere of radius r"""
    t = verts.astype(np.float64)[faces]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return float(r - (np.abs((n * t[:, 0]).sum(-1)) / np.linalg.norm(n, axis=-1)).min())


@functools.lru_cache(None)
def mesh(name):
    """verts (V,3) float32, faces (F,3) int32, centre (3,), r_in, r_out"""
    if name == "cube":
        v, f = cube()
        return v, f, (CUBE_LO + CUBE_HI) / 2, 0.5, 0.5 * 3 ** 0.5
    v, f = icosphere() if name == "icosphere" else hemisphere()
    return v, f, np.zeros(3), 0.3 - sagitta(*icosphere(), 0.3), 0.3


MESHES = ("cube", "icosphere", "hemisphere")


def default_aabb(verts):
    """lab4d_amd.meshray.default_aabb restated in numpy float32: the bounds widened by 2^-10 of each extent (of the largest on an axis with none)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    v = v[np.isfinite(v).all(1)]
    lo, hi = v.min(0), v.max(0)
    ext = hi - lo
    margin = np.where(ext > 0, ext, ext.max() if ext.max() > 0 else np.float32(1)).astype(np.float32) * PAD
    return np.stack([lo - margin, hi + margin]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------
def impact(o, d, centre):
    """(R,) float64: distance of the centre from the ray's line"""
    o, d = o.astype(np.float64), d.astype(np.float64)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    w = centre[None] - o
    return np.linalg.norm(w - (w * u).sum(-1, keepdims=True) * u, axis=-1)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(None)
def rays(name, kind, n, seed=0):
    """origin, dir (n,3), t_range (n,2) float32 of the HIT / MISS / INSIDE set of a mesh"""
    _, _, centre, r_in, r_out = mesh(name)
    rng = np.random.default_rng(1000 * seed + {"hit": 1, "miss": 2, "inside": 3}[kind] + 10 * MESHES.index(name))
    m = 8 * n + 64
    ball = _unit(rng, m) * rng.random((m, 1)) ** (1 / 3)
    if kind == "inside":
        o = centre + 0.5 * r_in * ball
        d = _unit(rng, m) * rng.uniform(0.5, 2.0, (m, 1))
        keep = np.ones(m, bool)
    else:
        o = centre + 3 * r_out * _unit(rng, m)
        target = centre + (0.8 * r_in * ball if kind == "hit" else 2.5 * r_out * ball)
        d = target - o
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (m, 1))
        b = impact(o.astype(np.float32), d.astype(np.float32), centre)
        keep = b <= 0.8 * r_in if kind == "hit" else b >= 1.3 * r_out
    o, d = o[keep][:n].astype(np.float32), d[keep][:n].astype(np.float32)
    assert o.shape[0] == n, (kind, int(keep.sum()))
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    tr = np.stack([np.zeros(n), 5 * r_out / ln], 1).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(tr)


@functools.lru_cache(None)
def mixed_rays(name, n=1025):
    """hit, miss and inside rays interleaved (shared, never modified)"""
    sets = [rays(name, "hit", n, seed=1), rays(name, "miss", n, seed=1), rays(name, "inside", n, seed=1)]
    pick = np.arange(n) % 3
    return tuple(np.ascontiguousarray(np.where((pick == 0)[:, None], sets[0][i], np.where((pick == 1)[:, None], sets[1][i], sets[2][i]))) for i in range(3))


# ---------------------------------------------------------------------------------------------------
# truth: float64 Moeller-Trumbore over all faces
# ---------------------------------------------------------------------------------------------------
def truth(verts, faces, o, d, tr, chunk=128):
    """dict: t (R,) float64 (nan without a hit), face (R,) (-1), hit, runner_up (R,): the second smallest t (inf), front (R,) bool: the ray meets
    the side (b - a) x (c - a) points to"""
    tri = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    a, e1, e2 = tri[None, :, 0], (tri[:, 1] - tri[:, 0])[None], (tri[:, 2] - tri[:, 0])[None]
    R, F = o.shape[0], faces.shape[0]
    t_all = np.full((R, F), np.inf)
    for s in range(0, R, chunk):
        oo, dd = o[s:s + chunk, None].astype(np.float64), d[s:s + chunk, None].astype(np.float64)
        with np.errstate(all="ignore"):
            h = np.cross(dd, e2)
            det = (e1 * h).sum(-1)
            sv = oo - a
            u = (sv * h).sum(-1) / det
            q = np.cross(sv, e1)
            v = (dd * q).sum(-1) / det
            t = (e2 * q).sum(-1) / det
            ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= tr[s:s + chunk, :1]) & (t <= tr[s:s + chunk, 1:])
        t_all[s:s + chunk] = np.where(ok, t, np.inf)
    if F == 0:
        return {"t": np.full(R, np.nan), "face": np.full(R, -1), "hit": np.zeros(R, bool), "runner_up": np.full(R, np.inf), "front": np.zeros(R, bool)}
    face = t_all.argmin(1)
    t = t_all[np.arange(R), face]
    hit = np.isfinite(t)
    n = np.cross(e1[0], e2[0])[face]
    return {"t": np.where(hit, t, np.nan), "face": np.where(hit, face, -1), "hit": hit, "front": (n * d.astype(np.float64)).sum(-1) < 0,
            "runner_up": np.partition(t_all, 1, axis=1)[:, 1] if F > 1 else np.full(R, np.inf)}


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def _aligned(n, dtype):
    """n elements of dtype on a 16-byte boundary (the packed faces are read as 16-byte words)"""
    raw = np.zeros(n * np.dtype(dtype).itemsize + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * np.dtype(dtype).itemsize].view(dtype)


def host_build(lib, verts, faces, G, aabb=None, expect_ok=True):
    """the twin's grid: dict with tris (F,12), cell_start, cell_list, aabb (6,), G, F"""
    verts, faces = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    aabb = np.ascontiguousarray(default_aabb(verts) if aabb is None else aabb, np.float32).reshape(-1)
    F = faces.shape[0]
    tris = _aligned(max(F, 1) * 12, np.float32)
    cell_start = np.full(max(G, 1) ** 3 + 1, -7, np.int32)
    head = (_ptr(verts), _ptr(faces), verts.shape[0], F, aabb.ctypes.data, G, tris.ctypes.data, cell_start.ctypes.data)
    total = lib.meshray_host_build(*head, None)
    if not expect_ok:
        assert total == -1, total
        return None
    assert total >= 0 and total == cell_start[-1], total
    cell_list = np.full(total, -7, np.int32)
    assert lib.meshray_host_build(*head, _ptr(cell_list)) == total
    return {"tris": tris[:F * 12].reshape(F, 12), "tris_buf": tris, "cell_start": cell_start, "cell_list": cell_list, "aabb": aabb, "G": G, "F": F}


def host_cast(lib, grid, o, d, tr, expect=0):
    o, d, tr = (np.ascontiguousarray(x, np.float32) for x in (o, d, tr))
    R = o.shape[0]
    out = {"t": np.full(R, 7.0, np.float32), "face": np.full(R, -7, np.int32), "u": np.full(R, 7.0, np.float32), "v": np.full(R, 7.0, np.float32),
           "front": np.full(R, -7, np.int32), "n_tests": np.full(R, -7, np.int32)}
    rc = lib.meshray_host_cast(_ptr(o), _ptr(d), _ptr(tr), R, grid["tris_buf"].ctypes.data, grid["F"], grid["aabb"].ctypes.data, grid["G"],
                               grid["cell_start"].ctypes.data, _ptr(grid["cell_list"]), *[_ptr(out[k]) for k in ("t", "face", "u", "v", "front", "n_tests")])
    assert rc == expect, rc
    return out


def lists_of(cell_start, cell_list):
    """{cell: sorted faces} of the non-empty cells"""
    cell_start, cell_list = np.asarray(cell_start), np.asarray(cell_list)
    return {int(c): sorted(cell_list[cell_start[c]:cell_start[c + 1]].tolist()) for c in np.nonzero(np.diff(cell_start))[0]}


def ref_lists(tris, aabb, G):
    """the GRID rule restated in numpy float32 over packed faces (tris (F,12): validity in column 3): {cell: sorted faces}"""
    out = {}
    lo, ext = aabb[:3].astype(np.float32), (aabb[3:] - aabb[:3]).astype(np.float32)
    for f, rec in enumerate(np.asarray(tris, np.float32).reshape(-1, 12)):
        if rec[3] == 0:
            continue
        p = rec.reshape(3, 4)[:, :3]
        with np.errstate(all="ignore"):
            g0 = np.floor(((p.min(0) - lo) / ext).astype(np.float32) * np.float32(G) - PAD)
            g1 = np.floor(((p.max(0) - lo) / ext).astype(np.float32) * np.float32(G) + PAD)
        if not ((g1 >= 0) & (g0 <= G - 1)).all():
            continue
        i0, i1 = np.maximum(g0, 0).astype(int), np.minimum(g1, G - 1).astype(int)
        for z in range(i0[2], i1[2] + 1):
            for y in range(i0[1], i1[1] + 1):
                for x in range(i0[0], i1[0] + 1):
                    out.setdefault(x + G * (y + G * z), []).append(f)
    return out


# ---------------------------------------------------------------------------------------------------
# the degenerate rays of the rules, on the cube under its default box (every value dyadic: the expected t is exact)
# ---------------------------------------------------------------------------------------------------
def degenerate_rays():
    """origin, dir, t_range (float32) and want: ('hit', t, face or None, front), 'untested' (face -1, t = t0, n_tests 0: rejected or clipped away) or
    'miss' (face -1, t = t0)"""
    nan, inf = float("nan"), float("inf")
    ok_o, ok_d = (0.125, 0.5, -2), (0, 0, 1)
    rows = [((0, 0.25, -2), (0, 0, 1), (0, 4), ("hit", 1.25, 0, 1)),          # axis-parallel, onto the diagonal shared by faces 0 and 1: the lower index
            ((2, 0.375, -0.125), (-2, 0, 0), (0, 4), ("hit", 0.75, None, 1)),  # axis-parallel, |d| = 2
            ((-2, 0.375, -0.125), (-1, 0, 0), (-4, 0), ("hit", -2.5, None, 1)),  # negative t: the far side comes first
            (ok_o, (0, 0, 0), (0, 4), "untested"),                             # d = 0
            (ok_o, (0, 0, 1e-30), (0, 4), "untested"),                         # len underflows to 0
            ((nan, 0.5, -2), ok_d, (0, 4), "untested"), ((0.125, inf, -2), ok_d, (0, 4), "untested"), ((0.125, 0.5, -inf), ok_d, (0, 4), "untested"),
            (ok_o, (nan, 0, 1), (0, 4), "untested"), (ok_o, (0, inf, 1), (0, 4), "untested"), (ok_o, (0, 0, -inf), (0, 4), "untested"),
            (ok_o, ok_d, (nan, 4), "untested"), (ok_o, ok_d, (0, nan), "untested"), (ok_o, ok_d, (-inf, 4), "untested"), (ok_o, ok_d, (0, inf), "untested"),
            (ok_o, ok_d, (3, 2), "untested"),                                  # t0 > t1
            (ok_o, ok_d, (1.25, 1.25), ("hit", 1.25, None, 1)),                # t0 == t1 on the surface
            (ok_o, ok_d, (1.5, 1.5), "miss"),                                  # t0 == t1 inside the cube, off the surface
            (ok_o, ok_d, (1.0, 1.0), "untested"),                              # t0 == t1 in front of the box: an empty clip
            ((0, 0.5, -2), ok_d, (0, 4), ("hit", 1.25, None, 1)),              # along the cell face x = 0 of G = 2
            ((-2, -1.75, -2.25), (1, 1, 1), (0, 4), ("hit", 1.5, 0, 1)),       # the box's diagonal: onto a vertex of the cube, through the grid corner of G = 2
            ((3, 0.5, -2), ok_d, (0, 4), "untested"),                          # a box miss, the parallel axes outside
            ((0, 0.25, -2), (0.3, 0.3, -1), (0, 4), "untested"),               # a box miss, pointing away
            ((0.125, 0.5, -0.25), (1, 0, 0), (0, 4), ("hit", 0.375, None, 0)),  # origin inside the box and the cube: a back face
            ((0.125, 0.5, -0.25), (1, 0, 0), (0, 0.25), "miss")]               # ... and a range that ends before it
    o, d, tr = (np.array([r[i] for r in rows], np.float32) for i in range(3))
    return o, d, tr, [r[3] for r in rows]


def check_degenerate(out):
    o, d, tr, want = degenerate_rays()
    for r, w in enumerate(want):
        got = {k: out[k][r].item() for k in out}
        if isinstance(w, tuple):
            assert got["face"] >= 0 and got["t"] == w[1] and got["front"] == w[3] and got["n_tests"] >= 1, (r, got)
            assert w[2] is None or got["face"] == w[2], (r, got)
            assert 0 <= got["u"] <= 1 and 0 <= got["v"] <= 1 and got["u"] + got["v"] <= 1 + 1e-6, (r, got)
        else:
            same_t = got["t"] == float(tr[r, 0]) or (np.isnan(got["t"]) and np.isnan(tr[r, 0]))
            assert got["face"] == -1 and same_t and got["u"] == 0 and got["v"] == 0 and got["front"] == 0, (r, got)
            assert got["n_tests"] == 0 if w == "untested" else got["n_tests"] >= 0, (r, got)


def same_hits(a, b, keys=("t", "face", "u", "v", "front")):
    """word for word (NaN == NaN by its bits)"""
    return all(np.array_equal(np.asarray(a[k]).view(np.int32), np.asarray(b[k]).view(np.int32)) for k in keys)
