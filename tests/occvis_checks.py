"""Shared by tests/test_occvis_host.py (CPU twin against numpy in float64) and tests/test_gpu_zzzzzzzzzzzzzzzzzoccvis.py (kernels against the
twin, word for word): the host harness of the visibility cull (tests/host_harness/occvis/occvis_host.cpp over lab4d_amd/csrc/occvis_math.hpp),
the camera sets, and the rules of include/lab4d_occvis.h restated in numpy float64 (vectorised; shares no code with the header).  The grid
helpers are those of tests/occgrid_checks.py and tests/conemarch_checks.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conemarch_checks as CC  # noqa: E402
import host_twin  # noqa: E402
import occgrid_checks as OC  # noqa: E402

TWIN = "occvis/occvis"  # tests/host_harness/occvis/occvis_host.cpp
SLACK = 16.0 * 2.0 ** -23
WH = (64, 48)


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
def host_sees(lib, planes, aabbs, G):
    """(K, G^3, M) bool: SEES per (cell, view)"""
    planes, aabbs = _c(planes, np.float32), _c(aabbs, np.float32)
    M, K = planes.shape[0], aabbs.shape[0]
    out = np.full((K, G ** 3, M), 9, np.uint8)
    lib.occvis_host_sees(planes.ctypes.data, M, aabbs.ctypes.data, K, G, out.ctypes.data)
    assert out.max() <= 1
    return out.astype(bool)


def host_mark(lib, planes, aabbs, G, min_views):
    """(vis_bits (K, words) uint32, n_visible (K,) int32)"""
    planes, aabbs = _c(planes, np.float32), _c(aabbs, np.float32)
    M, K = planes.shape[0], aabbs.shape[0]
    bits, n = np.full((K, OC.n_words(G)), 0xDEADBEEF, np.uint32), np.full(K, -7, np.int32)
    lib.occvis_host_mark(planes.ctypes.data, M, aabbs.ctypes.data, K, G, min_views, bits.ctypes.data, n.ctypes.data)
    return bits, n


def host_apply(lib, vis_bits, ema, bits, G):
    """in place on ema (K, G^3) float32 and bits (K, words) uint32; returns n_occupied (K,)"""
    vis_bits = _c(vis_bits, np.uint32)
    K = vis_bits.shape[0]
    assert ema.dtype == np.float32 and bits.dtype == np.uint32 and ema.shape == (K, G ** 3) and bits.shape == vis_bits.shape
    n = np.full(K, -7, np.int32)
    lib.occvis_host_apply(vis_bits.ctypes.data, ema.ctypes.data, bits.ctypes.data, n.ctypes.data, K, G)
    return n


# ---------------------------------------------------------------------------------------------------
# cameras
# ---------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """field2cam (4, 4) float64 of a camera at `eye` whose +z axis points at `target` (x right, y down): x_cam = R x_field + t"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, np.asarray(up, np.float64))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def intrinsics(M, focal=60.0, wh=WH):
    return np.tile(np.array([focal, focal * 1.1, wh[0] / 2 + 1.5, wh[1] / 2 - 2.0]), (M, 1))


def ring(M, centre, radius, height=0.3, phase=0.1):
    """M cameras on a circle of `radius` around `centre`, lifted by height * radius, looking at the centre"""
    a = phase + 2 * np.pi * np.arange(M) / M
    eyes = centre + radius * np.stack([np.cos(a), np.sin(a), np.full(M, height)], 1)
    return np.stack([look_at(e, centre) for e in eyes])


def camera_groups(base=OC.AABB, n_ring=6):
    """The camera sets as a list of dicts(Kmat (M,4), E (M,4,4), wh, near, far, pad) float64 over the box `base` and its cascade: a ring looking
    at the centre; views inside the box; one looking away (sees nothing of the base box); one with a NaN pose; a near plane that cuts the box;
    a finite far that cuts it."""
    lo, hi = base[0].astype(np.float64), base[1].astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    r = float(np.linalg.norm(half))
    groups = [dict(E=ring(n_ring, mid, 3.0 * r), near=0.05 * r, far=None, pad=0.0)]
    inside = np.stack([look_at(mid + half * np.array([0.31, -0.22, 0.13]), mid + half * np.array([-3.0, 0.7, 0.4])),
                       look_at(mid + half * np.array([-0.52, 0.41, -0.33]), mid + half * np.array([0.2, 2.5, 1.0])),
                       look_at(mid + half * np.array([0.05, 0.02, 0.61]), mid + half * np.array([0.3, -0.2, -4.0]), up=(0.0, 1.0, 0.0))])
    groups.append(dict(E=inside, near=0.02 * r, far=None, pad=2.0))
    away = look_at(mid + np.array([40.0 * r, 0.0, 0.0]), mid + np.array([80.0 * r, 1.0, 0.5]))[None]
    groups.append(dict(E=away, near=0.05 * r, far=None, pad=0.0))
    nan_pose = look_at(mid + np.array([0.0, 3.0 * r, 0.2 * r]), mid)[None].copy()
    nan_pose[0, 1, 3] = np.nan
    groups.append(dict(E=nan_pose, near=0.05 * r, far=None, pad=0.0))
    cut = look_at(mid + np.array([0.0, -2.0 * r, 0.5 * r]), mid)[None]
    groups.append(dict(E=cut, near=2.0 * r, far=None, pad=0.0))  # the near plane passes near the centre
    fin = np.stack([look_at(mid + np.array([2.5 * r, 0.3 * r, -0.4 * r]), mid), look_at(mid + np.array([-1.0 * r, 2.0 * r, 1.0 * r]), mid)])
    groups.append(dict(E=fin, near=0.1 * r, far=2.6 * r, pad=0.0))
    for g in groups:
        g.update(Kmat=intrinsics(g["E"].shape[0]), wh=WH)
    return groups


def planes_f64(Kmat, E, wh, near, far=None, pad=0.0):
    """VIEWS and CAMERA of include/lab4d_occvis.h in numpy float64: (M, 6, 4), not rounded"""
    Kmat, E = np.asarray(Kmat, np.float64), np.asarray(E, np.float64)
    M = Kmat.shape[0]
    fx, fy, cx, cy = Kmat.T
    W, H = float(wh[0]), float(wh[1])
    z, o = np.zeros(M), np.ones(M)
    cam = [(fx, z, cx + pad, z), (-fx, z, W + pad - cx, z), (z, fy, cy + pad, z), (z, -fy, H + pad - cy, z), (z, z, o, z - near)]
    if far is not None:
        cam.append((z, z, -o, z + far))
    cam = np.stack([np.stack(p, -1) for p in cam], 1)
    with np.errstate(invalid="ignore"):
        cam = cam / np.sqrt(cam[..., 0] * cam[..., 0] + cam[..., 1] * cam[..., 1] + cam[..., 2] * cam[..., 2])[..., None]
        R, t = E[:, :3, :3], E[:, :3, 3]
        n = [R[:, None, 0, i] * cam[..., 0] + R[:, None, 1, i] * cam[..., 1] + R[:, None, 2, i] * cam[..., 2] for i in range(3)]
        d = cam[..., 0] * t[:, None, 0] + cam[..., 1] * t[:, None, 1] + cam[..., 2] * t[:, None, 2] + cam[..., 3]
    out = np.stack(n + [d], -1)
    if far is None:
        out = np.concatenate([out, np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (M, 1, 1))], 1)
    return out


def all_planes(groups):
    """(planes float64 (M, 6, 4), planes float32): the groups' views in one list"""
    p = np.concatenate([planes_f64(g["Kmat"], g["E"], g["wh"], g["near"], g["far"], g["pad"]) for g in groups])
    return p, p.astype(np.float32)


TILE = 64  # lab4d_occvis::kTile, the views per LDS tile of the kernel


def seeing_slots(M):
    """the positions of the views that see something in tile_views(M): the first view, three further ones below the middle, the last two, and the
    views on both sides of every tile edge"""
    edges = [p for b in range(TILE, M, TILE) for p in (b - 1, b, b + 1)]
    return sorted({p for p in [0, M // 5, M // 3, M // 2, M - 2, M - 1] + edges if 0 <= p < M})


def tile_views(M, base=OC.AABB):
    """(M, 6, 4) float32 whose marks depend on every tile and on min_views: the slots of seeing_slots(M) hold DISTINCT views from
    inside the box, each seeing another part of it (seeded by the slot), every other slot a view that sees nothing -- the NaN pose, and the
    view looking away at every eighth slot.  A cell's count of views therefore rises across the tile edges."""
    lo, hi = base[0].astype(np.float64), base[1].astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    r = float(np.linalg.norm(half))
    groups = camera_groups(base)
    away, nan_pose = all_planes([groups[2]])[1][0], all_planes([groups[3]])[1][0]
    out = np.stack([away if m % 16 == 3 else nan_pose for m in range(M)])
    for m in seeing_slots(M):
        rng = np.random.default_rng(1000 + m)
        eye = mid + half * rng.uniform(-0.25, 0.25, 3)
        d = rng.standard_normal(3)
        E = look_at(eye, eye + d / np.linalg.norm(d), up=(0.3, 0.2, 1.0))[None]
        out[m] = planes_f64(intrinsics(1, focal=25.0), E, WH, 0.02 * r, None, 0.0).astype(np.float32)[0]
    return out


def repeat_views(planes32, M):
    """M views out of a set, cycling through it, with the non-finite view kept among the first ones"""
    return planes32[np.arange(M) % planes32.shape[0]]


# ---------------------------------------------------------------------------------------------------
# the rule in float64
# ---------------------------------------------------------------------------------------------------
def cell_boxes_f64(box, G):
    """(c (G^3, 3), h (3,)) of one level's box (6,) float32, exact in float64, x slowest"""
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    h = (hi - lo) / (2 * G)
    i = np.arange(G)
    I, J, L = np.meshgrid(i, i, i, indexing="ij")
    cell = np.stack([I, J, L], -1).reshape(-1, 3)
    return lo + (2 * cell + 1) * h, h


def classify_f64(planes64, aabbs, G):
    """(sure_seen, sure_not) (K, G^3, M) bool: with v_p = n.c + |n|.h + d and slack_p = 16 * 2^-23 * (sum |n_a| (|c_a| + h_a) + |d|) per
    plane in float64, a view surely sees a cell if every v_p >= 0 and surely does not if some v_p < -2 slack_p or a coefficient of the view
    is not finite; in between either answer is allowed"""
    K, M = aabbs.shape[0], planes64.shape[0]
    seen, sure_not = np.zeros((K, G ** 3, M), bool), np.zeros((K, G ** 3, M), bool)
    for lv in range(K):
        c, h = cell_boxes_f64(aabbs[lv], G)
        q = np.abs(c) + h
        for m in range(M):
            P = planes64[m]
            if not np.isfinite(P).all():
                sure_not[lv, :, m] = True
                continue
            n, d = P[:, :3], P[:, 3]
            v = c @ n.T + np.abs(n) @ h + d  # (G^3, 6)
            slack = SLACK * (q @ np.abs(n).T + np.abs(d))
            seen[lv, :, m] = (v >= 0).all(1)
            sure_not[lv, :, m] = (v < -2 * slack).any(1)
    return seen, sure_not


def points_seen_f64(pts, g):
    """(n, M) bool: the float64 point projects into the image of view m of group g at near <= z <= far (no pad: the bare image)"""
    E, Kmat = g["E"], g["Kmat"]
    W, H = g["wh"]
    with np.errstate(invalid="ignore", divide="ignore"):
        xc = np.einsum("mij,nj->nmi", E[:, :3, :3], pts) + E[None, :, :3, 3]
        z = xc[..., 2]
        u = Kmat[None, :, 0] * xc[..., 0] / z + Kmat[None, :, 2]
        v = Kmat[None, :, 1] * xc[..., 1] / z + Kmat[None, :, 3]
        ok = (z >= g["near"]) & (u >= 0) & (u <= W) & (v >= 0) & (v <= H)
        if g["far"] is not None:
            ok &= z <= g["far"]
    return ok


def unpack_levels(words, G):
    return np.stack([OC.unpack(w, G) for w in np.ascontiguousarray(words).view(np.uint32)])


def raise_to_parents(vis):
    """(K, G, G, G) bool: level c raised to contain the parents of level c - 1's set cells (CC.parent_index)"""
    vis = vis.copy()
    K, G = vis.shape[0], vis.shape[1]
    j = CC.parent_index(G)
    I, J, L = np.meshgrid(j, j, j, indexing="ij")
    for c in range(1, K):
        np.logical_or.at(vis[c], (I, J, L), vis[c - 1])
    return vis
