"""Shared by tests/test_meshsdf_host.py (CPU twin against float64) and tests/test_gpu_zzzzzzmeshsdf.py (kernels against the twin): the host
harness of the mesh distance (tests/host_harness/meshsdf_host.cpp over lab4d_amd/csrc/meshsdf_math.hpp), the test meshes, and the rules
of include/lab4d_meshsdf.h restated in numpy float64: the same region classification, the same winding formula."""
import functools

import numpy as np

import host_twin

EPS32 = float(np.finfo(np.float32).eps)


def build_host():
    return host_twin.load("meshsdf")


def host_query(lib, verts, faces, pts, n_slices=None):
    """The twin: dict with sdf, d2, wsum (the sum of the atan2 terms: w = wsum / 2 pi), face, closest.  n_slices: the sliced variant."""
    verts, pts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    faces = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    N = pts.shape[0]
    out = {"sdf": np.full(N, 7.0, np.float32), "d2": np.full(N, 7.0, np.float32), "wsum": np.full(N, 7.0, np.float32), "face": np.full(N, -7, np.int32),
           "closest": np.full((N, 3), 7.0, np.float32)}
    tail = [out[k].ctypes.data for k in ("sdf", "d2", "wsum", "face", "closest")]
    head = [verts.ctypes.data, faces.ctypes.data, verts.shape[0], faces.shape[0], pts.ctypes.data, N]
    if n_slices is None:
        lib.meshsdf_host_query(*head, *tail)
    else:
        lib.meshsdf_host_query_sliced(*head, int(n_slices), *tail)
    return out


def host_valid(lib, verts, faces):
    verts, faces = np.ascontiguousarray(verts, np.float32).reshape(-1, 3), np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    out = np.full(faces.shape[0], 7, np.uint8)
    lib.meshsdf_host_valid(verts.ctypes.data, faces.ctypes.data, verts.shape[0], faces.shape[0], out.ctypes.data)
    return out.astype(bool)


# ---------------------------------------------------------------------------------------------------
# meshes
# ---------------------------------------------------------------------------------------------------
CUBE_LO, CUBE_HI = np.array([-0.5, -0.25, -0.75]), np.array([0.5, 0.75, 0.25])  # dyadic corners: the constructed ties are exact


def cube():
    """12 triangles, outward; faces 2k and 2k + 1 share the diagonal of one side"""
    c = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64)
    verts = (CUBE_LO + c * (CUBE_HI - CUBE_LO)).astype(np.float32)
    faces = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [3, 7, 6], [3, 6, 2], [0, 4, 7], [0, 7, 3], [1, 2, 6], [1, 6, 5]], np.int32)
    return verts, faces


def box_distance(pts):
    """analytic unsigned distance to the cube's SURFACE, float64"""
    p = np.asarray(pts, np.float64)
    q = np.maximum(np.maximum(CUBE_LO - p, p - CUBE_HI), 0.0)
    outside = np.sqrt((q ** 2).sum(-1))
    inside = np.minimum(p - CUBE_LO, CUBE_HI - p).min(-1)
    return np.where((q > 0).any(-1), outside, inside)


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


def sagitta(verts, faces, r):
    """how far the flat faces dip below the sphere of radius r: r - the smallest distance of a face's plane from the centre"""
    t = verts.astype(np.float64)[faces]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    h = np.abs((n * t[:, 0]).sum(-1)) / np.linalg.norm(n, axis=-1)
    return float(r - h.min())


def hemisphere(level=3, r=0.3):
    """the faces of the icosphere whose centroid has z > 0: open, with a ragged rim"""
    v, f = icosphere(level, r)
    keep = v[f].mean(1)[:, 2] > 0
    return v, f[keep]


def flipped(faces):
    return np.ascontiguousarray(faces[:, ::-1])


def bbox_diagonal(verts, pts):
    allp = np.concatenate([np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(pts, np.float64).reshape(-1, 3)])
    allp = allp[np.isfinite(allp).all(-1)]
    return float(np.linalg.norm(allp.max(0) - allp.min(0)))


def d2_bound(L):
    """|d2_fp32 - d2_exact| <= 64 * eps32 * L^2: about twenty rounded operations (three differences and three products per dot product, the
    quotient, the point on the edge or face, the final difference and its square) on quantities of at most L^2, each within eps32 / 2 of
    its exact value, with a margin of 3.  A tangential error of the closest point moves d2 in second order only (Pythagoras)."""
    return 64 * EPS32 * L * L


def points_around(verts, n, seed, scale=1.5):
    """uniform in the mesh's bounding box scaled by `scale` about its centre"""
    v = np.asarray(verts, np.float64)
    lo, hi = v.min(0), v.max(0)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * scale
    return (c + (np.random.default_rng(seed).random((n, 3)) * 2 - 1) * h).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# the rules in float64
# ---------------------------------------------------------------------------------------------------
def ref_valid(verts, faces):
    verts, faces = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    in_range = ((faces >= 0) & (faces < verts.shape[0])).all(-1)
    t = verts[np.where(in_range[:, None], faces, 0)] if verts.shape[0] else np.zeros((faces.shape[0], 3, 3))
    with np.errstate(all="ignore"):
        n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        n2 = (n ** 2).sum(-1)
    return in_range & np.isfinite(t).all((1, 2)) & np.isfinite(n2) & (n2 > 0) & (n2 < 3.4e38)


def ref_query(verts, faces, pts, chunk=256):
    """float64 brute force over the VALID faces: dict with d2_all (N, F; +inf for invalid faces), q_all's winner `closest`, face (argmin,
    lowest index first), d2, runner_up (the second smallest d2), w (the winding number), sdf."""
    verts, pts = np.asarray(verts, np.float64).reshape(-1, 3), np.asarray(pts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ref_valid(verts, faces)
    F, N = faces.shape[0], pts.shape[0]
    tri = verts[np.where(ok[:, None], faces, 0)] if verts.shape[0] else np.zeros((F, 3, 3))
    tri = np.where(ok[:, None, None], tri, 0.0)
    d2_all, q_all, w = np.full((N, F), np.inf), np.zeros((N, F, 3)), np.zeros(N)
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    ab, ac = b - a, c - a
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    for o in range(0, N, chunk):
        p = pts[o:o + chunk, None, :]
        with np.errstate(all="ignore"):
            ap, bp, cp = p - a, p - b, p - c
            d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                     (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
            s = va + vb + vc
            cands = [a + 0 * p, b + 0 * p, a + (d1 / (d1 - d3))[..., None] * ab, c + 0 * p, a + (d2 / (d2 - d6))[..., None] * ac,
                     b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b), a + ab * (vb / s)[..., None] + ac * (vc / s)[..., None]]
            q = cands[6]
            for cond, cand in list(zip(conds, cands))[::-1]:
                q = np.where(cond[..., None], cand, q)
            dd = ((p - q) ** 2).sum(-1)
            va_, vb_, vc_ = -ap, -bp, -cp  # vertex - p
            la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (va_, vb_, vc_))
            det = dot(va_, np.cross(vb_, vc_))
            den = la * lb * lc + dot(va_, vb_) * lc + dot(vb_, vc_) * la + dot(vc_, va_) * lb
            w[o:o + chunk] = np.where(ok[None], 2 * np.arctan2(det, den), 0.0).sum(-1) / (4 * np.pi)
        d2_all[o:o + chunk] = np.where(ok[None], dd, np.inf)
        q_all[o:o + chunk] = q
    res = {"d2_all": d2_all, "q_all": q_all, "w": w, "valid": ok}
    if F and ok.any():
        face = d2_all.argmin(1)
        res["face"], res["d2"] = face, d2_all[np.arange(N), face]
        res["closest"] = q_all[np.arange(N), face]
        res["runner_up"] = np.partition(d2_all, 1, axis=1)[:, 1] if F > 1 else np.full(N, np.inf)
        res["sdf"] = np.where(np.abs(w) > 0.5, -1.0, 1.0) * np.sqrt(res["d2"])
    return res


def near_minimisers(ref, got_face, bound):
    """For the winning-face check.  Returns (got_in_near (N,): the face `got_face` names has a float64 d2 within `bound` of the point's
    float64 minimum; contested (N,): the float64 runner-up is within `bound` of the minimum, so float64 alone does not single out a face)."""
    N = ref["d2_all"].shape[0]
    ok = np.asarray(got_face) >= 0
    got_d2 = ref["d2_all"][np.arange(N), np.where(ok, got_face, 0)]
    return ok & (got_d2 <= ref["d2"] + bound), ref["runner_up"] <= ref["d2"] + bound
