"""Shared by tests/test_meshnear_host.py (CPU twin against the brute-force twin and float64) and tests/test_gpu_zzzzzzzzzzzzmeshnear.py (kernel
against the twin): the host harness of the grid distance query (tests/host_harness/meshnear/meshnear_host.cpp over
lab4d_amd/csrc/meshnear_math.hpp), the point sets, and the SIGN rule of include/lab4d_meshnear.h restated in numpy float64.  The meshes and
the grid's lists are those of tests/meshray_checks.py.  Everything built here is cached and shared between the two suites: never modified.

POINTS  per mesh, under its default box: 256 random points inside the box; 64 points each at 1, 8 and 1,024 box extents outside, cycling through
        the 26 side, edge and corner directions; every vertex, every edge midpoint and every face centroid (rounded to float32); the grid
        corners of G = 2 and G = 5 as the kernel computes its planes, and 64 points per G with one coordinate exactly on a cell wall."""
import functools
import os

import numpy as np

import host_twin
import meshray_checks as MC
import meshsdf_checks as SD

TWIN = "meshnear/meshnear"
SIZES_G = (1, 2, 5, 32)
OFF_SURFACE = 1e-5   # of the box diagonal L: where a sign is compared
S_MARGIN = 1e-4      # |s| > S_MARGIN |p - q| |n| on every point whose sign is compared: a condition on the inputs


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)
    return host_twin.load(TWIN)


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def host_closest(lib, grid, pts, sign_mode=1, orient=1, expect=0):
    """the twin on a grid of MC.host_build: dict of sdf, d2, face, closest, region, n_tests, n_cells"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    N = pts.shape[0]
    out = {"sdf": np.full(N, 7.0, np.float32), "d2": np.full(N, 7.0, np.float32), "face": np.full(N, -7, np.int32), "closest": np.full((N, 3), 7.0, np.float32),
           "region": np.full(N, -7, np.int32), "n_tests": np.full(N, -7, np.int32), "n_cells": np.full(N, -7, np.int32)}
    rc = lib.meshnear_host_closest(_ptr(pts), N, grid["tris_buf"].ctypes.data if grid["F"] else None, grid["F"], grid["aabb"].ctypes.data, grid["G"],
                                   grid["cell_start"].ctypes.data if grid["F"] else None, _ptr(grid["cell_list"]), sign_mode, orient,
                                   *[_ptr(out[k]) for k in ("sdf", "d2", "face", "closest", "region", "n_tests", "n_cells")])
    assert rc == expect, rc
    return out


def same_words(a, b, keys=("d2", "face", "closest", "region")):
    """word for word (NaN == NaN by its bits)"""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.int32), np.ascontiguousarray(b[k]).view(np.int32)) for k in keys)


def planes(box, G):
    """(3, G + 1) float32: the grid planes lo + (k / G) * ext as meshnear_math.hpp's plane_at rounds them"""
    lo, ext = box[0].astype(np.float32), (box[1] - box[0]).astype(np.float32)
    frac = (np.arange(G + 1, dtype=np.float32) / np.float32(G)).astype(np.float32)
    return (lo[:, None] + (frac[None] * ext[:, None]).astype(np.float32)).astype(np.float32)


DIRS = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], np.float64)


@functools.lru_cache(None)
def points(name, seed=0):
    """(N, 3) float32 and a dict of slices by kind"""
    verts, faces = MC.mesh(name)[:2]
    box = MC.default_aabb(verts).astype(np.float64)
    c, ext = (box[0] + box[1]) / 2, box[1] - box[0]
    rng = np.random.default_rng(7000 + 100 * seed + MC.MESHES.index(name))
    sets = {"inside": box[0] + rng.random((256, 3)) * ext}
    for k in (1, 8, 1024):
        d = DIRS[np.arange(64) % 26]
        sets["far%d" % k] = c + d * (0.5 + k) * ext + np.where(d == 0, rng.uniform(-0.45, 0.45, (64, 3)), d * rng.uniform(0, 0.3, (64, 3))) * ext
    v64 = verts.astype(np.float64)
    f = np.asarray(faces, np.int64)
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1), axis=0)
    sets["verts"], sets["edges"], sets["faces"] = v64[np.unique(f)], v64[edges].mean(1), v64[f].mean(1)
    for G in (2, 5):
        pl = planes(box.astype(np.float32), G).astype(np.float64)
        sets["corners%d" % G] = np.stack(np.meshgrid(pl[0], pl[1], pl[2], indexing="ij"), -1).reshape(-1, 3)
        w = box[0] + rng.random((64, 3)) * ext
        ax = np.arange(64) % 3
        w[np.arange(64), ax] = pl[ax, rng.integers(0, G + 1, 64)]
        sets["walls%d" % G] = w
    out, where, o = [], {}, 0
    for k, p in sets.items():
        where[k] = slice(o, o + p.shape[0])
        o += p.shape[0]
        out.append(p.astype(np.float32))
    return np.ascontiguousarray(np.concatenate(out)), where


def volume_orient(verts, faces):
    """MeshGrid.closest's orient="auto" restated in numpy float64: the sign of sum det[a - m, b - m, c - m] over the valid faces, m the mean of
    their corners; +1 for zero"""
    ok = SD.ref_valid(verts, faces)
    t = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)[ok]]
    if t.shape[0] == 0:
        return 1
    t = t - t.reshape(-1, 3).mean(0)
    return -1 if (t[:, 0] * np.cross(t[:, 1], t[:, 2])).sum() < 0 else 1


_FEATURE = {1: (0, 1), 2: (0, 2), 3: (1, 2), 4: (0,), 5: (1,), 6: (2,)}


def ref_side(verts, faces, pts, got):
    """The SIGN rule in float64 from the twin's face, region and closest point: s = (p - q) . n, with INCIDENT by equal coordinates over ALL valid
    faces (under a box that holds the mesh every incident face is listed in q's cell).  Returns s (N,), |p - q| |n| (N,), n_incident (N,)."""
    tri = np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]  # (F, 3, 3) float32: equality of coordinates is decided here
    ok = SD.ref_valid(verts, faces)
    t64 = tri.astype(np.float64)
    nrm = np.cross(t64[:, 1] - t64[:, 0], t64[:, 2] - t64[:, 0])
    with np.errstate(all="ignore"):
        unit = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    p, q = np.asarray(pts, np.float64).reshape(-1, 3), got["closest"].astype(np.float64)
    N = p.shape[0]
    s, scale, n_inc = np.zeros(N), np.zeros(N), np.zeros(N, int)
    for i in range(N):
        f, reg = int(got["face"][i]), int(got["region"][i])
        if f < 0:
            continue
        if reg == 0:
            n, n_inc[i] = nrm[f], 1
        else:
            fv = tri[f][list(_FEATURE[reg])]  # (1 or 2, 3)
            has = [(tri == v[None, None]).all(-1) for v in fv]  # each (F, 3)
            inc = ok & np.all([h.any(-1) for h in has], axis=0)
            n_inc[i] = inc.sum()
            if reg <= 3:
                n = unit[inc].sum(0)
            else:
                k = has[0][inc].argmax(-1)  # the face's first corner at the vertex
                ti = t64[inc]
                at = ti[np.arange(ti.shape[0]), k]
                e1, e2 = ti[np.arange(ti.shape[0]), (k + 1) % 3] - at, ti[np.arange(ti.shape[0]), (k + 2) % 3] - at
                ang = np.arctan2(np.linalg.norm(np.cross(e1, e2), axis=1), (e1 * e2).sum(-1))
                n = (ang[:, None] * unit[inc]).sum(0)
        s[i], scale[i] = ((p[i] - q[i]) * n).sum(), np.linalg.norm(p[i] - q[i]) * np.linalg.norm(n)
    return s, scale, n_inc


def check_outputs_sane(got, F):
    assert ((got["face"] >= -1) & (got["face"] < max(F, 1))).all() and ((got["region"] >= -1) & (got["region"] <= 6)).all()
    assert ((got["face"] < 0) == (got["region"] < 0)).all() and (got["n_tests"] >= 0).all()


def bad_cube():
    """the cube with four faces that are never listed in front (indices out of range, a NaN vertex, a degenerate face) and its box"""
    verts, faces = MC.cube()
    bv = np.concatenate([verts, np.array([[np.nan, 0, 0]], np.float32)])
    bf = np.concatenate([np.array([[0, 1, 99], [-1, 1, 2], [0, 1, 8], [5, 5, 6]], np.int32), faces])
    return bv, bf, MC.default_aabb(verts), 4
