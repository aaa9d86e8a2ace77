"""Shared by tests/test_mesh_host.py (CPU twin) and tests/test_gpu_zzzmesh.py (kernels): the host harness of the iso-surface extractor,
the test volumes, and the properties every correct welded iso-surface has.  No skimage exists here to compare with, so the mesh is pinned
by those properties (closed, manifold, consistently oriented, right Euler characteristic, vertices on the surface within the derived
interpolation bound) and by the ordering contract of include/lab4d_mesh.h restated independently in numpy."""
import importlib.util
import os

import numpy as np

import host_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def results_dir():
    """Where the device tests leave their measurement files: LAB4D_RESULTS_DIR, else the untracked results directory of this tree (the
    `*_out/` entry of .gitignore, where the other GPU tests write theirs)."""
    d = os.environ.get("LAB4D_RESULTS_DIR")
    if not d:
        names = [ln.strip().rstrip("/") for ln in open(os.path.join(ROOT, ".gitignore")) if ln.strip().endswith("_out/")]
        d = os.path.join(ROOT, names[0] if names else "results")
    os.makedirs(d, exist_ok=True)
    return d


def gen_module():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "tools", "gen_mc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_host():
    return host_twin.load("mesh")


def host_extract(lib, sdf, mask=None, level=0.0, origin=None, step=None):
    """(verts (V,3) f32, faces (F,3) i32) of the CPU twin; origin / step None = index space."""
    sdf = np.ascontiguousarray(sdf, np.float32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    xf = None if origin is None else np.ascontiguousarray(np.concatenate([np.asarray(origin, np.float32), np.asarray(step, np.float32)]), np.float32)
    counts = np.zeros(2, np.int32)
    args = (sdf.ctypes.data, None if m is None else m.ctypes.data, sdf.shape[0], sdf.shape[1], sdf.shape[2], float(level), None if xf is None else xf.ctypes.data)
    lib.mesh_host_extract(*args, None, None, 0, 0, counts.ctypes.data)
    verts, faces = np.empty((counts[0], 3), np.float32), np.empty((counts[1], 3), np.int32)
    lib.mesh_host_extract(*args, verts.ctypes.data, faces.ctypes.data, verts.shape[0], faces.shape[0], counts.ctypes.data)
    assert counts[0] == verts.shape[0] and counts[1] == faces.shape[0]
    return verts, faces


def host_largest_component(lib, verts, faces):
    verts, faces = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(faces, np.int32)
    ov, of, counts = np.empty_like(verts), np.empty_like(faces), np.zeros(2, np.int32)
    lib.mesh_host_largest_component(verts.ctypes.data, faces.ctypes.data, verts.shape[0], faces.shape[0], ov.ctypes.data, of.ctypes.data, counts.ctypes.data)
    return ov[:counts[0]].copy(), of[:counts[1]].copy()


# ---------------------------------------------------------------------------------------------------
# volumes
# ---------------------------------------------------------------------------------------------------
def random_volume(shape, seed):
    """Seeded normal noise (every ambiguous configuration occurs), border forced outside so that the surface is closed."""
    vol = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    vol[0] = vol[-1] = 1
    vol[:, 0] = vol[:, -1] = 1
    vol[:, :, 0] = vol[:, :, -1] = 1
    return vol


def grid_xyz(G):
    ax = np.linspace(-0.5, 0.5, G)
    return np.meshgrid(ax, ax, ax, indexing="ij")


def sphere(G, r=0.3, c=(0.0, 0.0, 0.0)):
    X, Y, Z = grid_xyz(G)
    return (np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - r).astype(np.float32)


def torus(G, R=0.28, r=0.1):
    X, Y, Z = grid_xyz(G)
    return (np.sqrt((np.sqrt(X ** 2 + Y ** 2) - R) ** 2 + Z ** 2) - r).astype(np.float32)


def two_spheres(G):
    """radius 0.15 around x = -0.22 (the larger: x in [-0.37, -0.07]) and radius 0.10 around x = +0.25 (x in [0.15, 0.35])"""
    return np.minimum(sphere(G, 0.15, (-0.22, 0, 0)), sphere(G, 0.10, (0.25, 0, 0)))


def three_blobs(G):
    """Two mirror-image spheres (the volume is mirrored, not recomputed: exactly equal sign patterns, hence a tie in vertex count) and a
    smaller third one between them.  The defined winner is the component holding the smallest vertex index: the one at low x (x is the
    slowest axis)."""
    left = sphere(G, 0.12, (-0.3, 0.05, 0.0))
    pair = np.minimum(left, left[::-1])
    return np.ascontiguousarray(np.minimum(pair, sphere(G, 0.07, (0.0, -0.25, 0.1))))


def world(G):
    """origin, step of the exact-spacing transform of a G^3 grid on [-0.5, 0.5]^3"""
    return np.full(3, -0.5, np.float32), np.full(3, 1.0 / (G - 1), np.float32)


# ---------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def unpaired_edges(faces, n_verts):
    """Directed edges that do not occur exactly once with their reverse exactly once (empty <=> closed, manifold, consistently oriented).
    Returns (rows into directed_edges(faces), number of directed edges that occur more than once)."""
    e = directed_edges(faces)
    key, rkey = e[:, 0] * n_verts + e[:, 1], e[:, 1] * n_verts + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    dup = int((cnt > 1).sum())
    has_rev = np.isin(rkey, uniq)
    return np.nonzero(~has_rev)[0], dup


def assert_closed(verts, faces):
    assert faces.shape[0] > 0
    assert faces.min() >= 0 and faces.max() < verts.shape[0]
    assert not ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])).any(), "a face repeats a vertex"
    open_rows, dup = unpaired_edges(faces, verts.shape[0])
    assert dup == 0 and open_rows.size == 0, (dup, open_rows.size)
    assert np.array_equal(np.unique(faces), np.arange(verts.shape[0])), "a vertex is referenced by no face"


def euler(verts, faces):
    e = np.sort(directed_edges(faces), 1)
    return verts.shape[0] - np.unique(e[:, 0] * verts.shape[0] + e[:, 1]).size + faces.shape[0]


def signed_volume(verts, faces):
    v = verts.astype(np.float64)[faces]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6)


def sphere_bound(G, r):
    """Largest distance of a vertex from the sphere: along a grid edge |d^2/ds^2 |p|| <= 1 / |p|, and the root of the linear interpolant
    is off by at most h^2 / 8 times that; |p| >= r - h on a crossed edge.  + 1e-6 for fp32."""
    h = 1.0 / (G - 1)
    return h * h / (8 * (r - h)) + 1e-6


# ---------------------------------------------------------------------------------------------------
# the contract of include/lab4d_mesh.h, restated in numpy (vectorised; shares no code with the harness or the kernels)
# ---------------------------------------------------------------------------------------------------
def meshed_cells(sdf, mask):
    """(Gx-1, Gy-1, Gz-1) bool: all 8 corners finite and unmasked."""
    ok = np.isfinite(sdf) if mask is None else (np.isfinite(sdf) & (np.asarray(mask) != 0))
    out = np.ones(tuple(g - 1 for g in sdf.shape), bool)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                out &= ok[di:di + sdf.shape[0] - 1, dj:dj + sdf.shape[1] - 1, dk:dk + sdf.shape[2] - 1]
    return out


def cell_cases(sdf, level):
    ins = (sdf < np.float32(level))
    G = sdf.shape
    case = np.zeros(tuple(g - 1 for g in G), np.int64)
    for c in range(8):
        di, dj, dk = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= ins[di:di + G[0] - 1, dj:dj + G[1] - 1, dk:dk + G[2] - 1].astype(np.int64) << c
    return case


def expected_vertices(sdf, mask, level):
    """Index-space vertices in contract order: ascending (linear index of the owning grid point) * 3 + axis; a vertex exists iff the edge
    is crossed and one of the cells around it is meshed and non-empty."""
    sdf = np.asarray(sdf, np.float32)
    G = sdf.shape
    level = np.float32(level)
    with np.errstate(invalid="ignore"):
        ins = sdf < level
    live = np.zeros(G, bool)  # per cell (stored at its low corner): meshed
    live[:-1, :-1, :-1] = meshed_cells(sdf, mask)
    lin = np.arange(sdf.size, dtype=np.int64).reshape(G)
    keys, pos = [], []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, G[a] - 1), slice(1, G[a])
        lo, hi = tuple(lo), tuple(hi)
        crossed = np.zeros(G, bool)
        crossed[lo] = ins[lo] != ins[hi]
        b, c = (a + 1) % 3, (a + 2) % 3
        near = np.zeros(G, bool)
        for db in (0, 1):
            for dc in (0, 1):
                sh = np.roll(live, (db, dc), axis=(b, c)).copy()
                if db:
                    idx = [slice(None)] * 3
                    idx[b] = 0
                    sh[tuple(idx)] = False
                if dc:
                    idx = [slice(None)] * 3
                    idx[c] = 0
                    sh[tuple(idx)] = False
                near |= sh
        on = crossed & near
        p = np.argwhere(on)
        va = sdf[on]
        nb = p.copy()
        nb[:, a] += 1
        vb = sdf[nb[:, 0], nb[:, 1], nb[:, 2]]
        t = (level - va) / (vb - va)
        q = p.astype(np.float32)
        q[:, a] = q[:, a] + t.astype(np.float32)
        keys.append(lin[on] * 3 + a)
        pos.append(q)
    keys, pos = np.concatenate(keys), np.concatenate(pos)
    order = np.argsort(keys, kind="stable")
    return pos[order]


def expected_face_cells(sdf, mask, level, tri_count):
    """(F, 3) integer cell coordinates of every face in contract order (ascending linear cell index, table count per cell)."""
    sdf = np.asarray(sdf, np.float32)
    with np.errstate(invalid="ignore"):
        case = np.where(meshed_cells(sdf, mask), cell_cases(sdf, level), 0)
    n = np.asarray(tri_count)[case]
    return np.repeat(np.argwhere(n >= 0), n.reshape(-1), axis=0)


def assert_matches_contract(verts_idx, faces, sdf, mask, level, tri_count):
    """Index-space output against the numpy restatement: vertex count, order and positions (exact or 1 ulp), face count, and every face
    inside the cell the ordering contract assigns it to."""
    exp = expected_vertices(sdf, mask, level)
    assert verts_idx.shape == exp.shape, (verts_idx.shape, exp.shape)
    assert np.isfinite(verts_idx).all()
    assert (np.abs(verts_idx - exp) <= np.spacing(np.abs(exp))).all(), float(np.abs(verts_idx - exp).max())
    assert (((verts_idx == np.round(verts_idx)).sum(1)) >= 2).all(), "a vertex must have two integer index coordinates"
    cells = expected_face_cells(sdf, mask, level, tri_count)
    assert faces.shape[0] == cells.shape[0], (faces.shape[0], cells.shape[0])
    if faces.shape[0]:
        tri = verts_idx[faces]  # (F, 3 corners, 3 axes)
        lo, hi = cells[:, None, :].astype(np.float32), cells[:, None, :].astype(np.float32) + 1
        assert ((tri >= lo) & (tri <= hi)).all(), "a face leaves the cell the ordering contract assigns it to"
