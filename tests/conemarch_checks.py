"""Shared by tests/test_conemarch_host.py (CPU twin against numpy) and tests/test_gpu_zzzzzzzzzzzzzzzzconemarch.py (kernels against the twin,
word for word): the host harness of the cone-stepped march through a cascade of occupancy grids
(tests/host_harness/conemarch/conemarch_host.cpp over lab4d_amd/csrc/conemarch_math.hpp), the test inputs, and the rules of
include/lab4d_conemarch.h restated twice in numpy -- in float32, operation by operation (numpy's float32 arithmetic is correctly rounded, so
the recurrence reproduces to the word), and in float64 for the kept set -- and the cascade's update rule in numpy.  The restatements are
vectorised over the rays and share no code with the header.  The grid and ray helpers are those of tests/occgrid_checks.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import occgrid_checks as OC  # noqa: E402

TWIN = "conemarch/conemarch"  # tests/host_harness/conemarch/conemarch_host.cpp: a folder of its own, as the other newer twins
F32_MAX = np.float32(3.402823466e+38)
DT_MIN, DT_MAX = 0.01, 0.16
CONES = (0.0, 1.0 / 256.0, 0.05)


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def cascade_boxes(K, base=OC.AABB):
    """(K, 6) float32: level c = centre +- half extent * 2^c of the base box, in float64, rounded once"""
    lo, hi = base[0].astype(np.float64), base[1].astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    return np.stack([np.concatenate([mid - half * 2.0 ** c, mid + half * 2.0 ** c]) for c in range(K)]).astype(np.float32)


def cascade_occupancy(K, G, seed, kind="random"):
    """(K, G, G, G) bool: independent per level (the kernels take the bits as given: no parent property here)"""
    if kind == "random":
        return np.stack([OC.random_occupancy(G, seed + 17 * c, 0.35) for c in range(K)])
    if kind == "full":
        return np.ones((K, G, G, G), bool)
    if kind == "empty":
        return np.zeros((K, G, G, G), bool)
    return np.stack([OC.sphere_occupancy(G, r=0.45 / 2 ** min(c, 2) + 0.1) for c in range(K)])  # a ball that shrinks with the level


def pack_levels(occ):
    return np.stack([OC.pack(o) for o in occ])


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
FIELDS = ("t", "steps", "deltas", "xyz", "dirs")


def host_march(lib, origin, direction, t_range, aabbs, bits, G, cone, dt_min, dt_max, k_max, cap=None, tail=0):
    """The twin's two passes around numpy's exclusive sum.  cap None: the total (nothing dropped).  `tail` further rows are allocated behind
    the cap and must keep their sentinels.  Returns a dict with the fields of lab4d_amd.packed.ConeRays (numpy; total an int, overflow a
    bool) and `count`, the untruncated per-ray counts."""
    origin, direction, t_range, aabbs = (_c(a, np.float32) for a in (origin, direction, t_range, aabbs))
    bits = _c(bits, np.uint32)
    R, K = origin.shape[0], aabbs.shape[0]
    assert bits.shape == (K, OC.n_words(G))
    count = np.zeros(R, np.int32)
    head = (origin.ctypes.data, direction.ctypes.data, t_range.ctypes.data, aabbs.ctypes.data, bits.ctypes.data, K, G, R, cone, dt_min, dt_max, k_max)
    lib.conemarch_host_count(*head, count.ctypes.data)
    incl = np.cumsum(count, dtype=np.int64)
    start = (incl - count).astype(np.int32)
    if cap is None:
        cap = int(incl[-1]) if R else 0
    n = cap + tail
    out = {"t": np.full(n, np.nan, np.float32), "steps": np.full(n, np.nan, np.float32), "deltas": np.full(n, np.nan, np.float32),
           "xyz": np.full((n, 3), np.nan, np.float32), "dirs": np.full((n, 3), np.nan, np.float32), "ray_idx": np.full(n, -7, np.int32),
           "level": np.full(n, -7, np.int32), "ray_count": np.full(R, -7, np.int32)}
    total, ovf = np.full(1, -7, np.int32), np.full(1, 7, np.uint8)
    lib.conemarch_host_write(*head, start.ctypes.data, cap, out["t"].ctypes.data, out["steps"].ctypes.data, out["deltas"].ctypes.data, out["xyz"].ctypes.data,
                             out["dirs"].ctypes.data, out["ray_idx"].ctypes.data, out["level"].ctypes.data, out["ray_count"].ctypes.data, total.ctypes.data,
                             ovf.ctypes.data)
    out.update(ray_start=start, total=int(total[0]), overflow=bool(ovf[0]), count=count, R=R, cap=cap)
    return out


def host_cascade_mask(lib, xyz, delta, aabbs, bits, G):
    """(mask (S,) uint8, level (S,) int32); delta None: the twin's NULL"""
    xyz, aabbs, bits = _c(xyz, np.float32), _c(aabbs, np.float32), _c(bits, np.uint32)
    delta = None if delta is None else _c(delta, np.float32)
    S = xyz.shape[0]
    mask, level = np.full(S, 9, np.uint8), np.full(S, -7, np.int32)
    lib.conemarch_host_cascade_mask(xyz.ctypes.data, None if delta is None else delta.ctypes.data, aabbs.ctypes.data, bits.ctypes.data, aabbs.shape[0], G, S,
                                    mask.ctypes.data, level.ctypes.data)
    return mask, level


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
N_SPECIAL = 16


def ray_set(aabbs, seed=5):
    """(origin (1025,3), dir (1025,3), t_range (1025,2)) float32 and the kinds of tests/occgrid_checks.py's rays, built against the OUTERMOST
    box (|d| from 0.5 to 2 box edges, axis-parallel rays, zero components, misses, origins inside the box), with 16 special rays in front so
    that every prefix R = 1 / 65 / 1025 holds them: the origin inside level 0, between two levels, outside box K - 1; non-finite values in each
    input; t0 > t1; t0 < 0; a ray grazing the face of an inner box; a miss; a zero direction."""
    K = aabbs.shape[0]
    outer = aabbs[K - 1].reshape(2, 3)
    o, d, tr, kinds = OC.rays(seed, aabb=outer)
    o, d, tr = o.copy(), d.copy(), tr.copy()
    lo0, hi0 = aabbs[0, :3].astype(np.float64), aabbs[0, 3:].astype(np.float64)
    mid, half0 = (lo0 + hi0) / 2, (hi0 - lo0) / 2
    ext = (outer[1] - outer[0]).astype(np.float64)
    gen = np.array([0.61, -0.43, 0.37]) * ext
    o[:N_SPECIAL], d[:N_SPECIAL], tr[:N_SPECIAL] = mid, gen, (0.0, 4.0)
    o[1] = mid + half0 * np.array([1.5, -0.2, 0.3]) * (1 if K > 1 else 0.5)  # between level 0 and level 1 (K = 1: inside)
    o[2, 1] = np.nan
    d[3, 2] = np.inf
    tr[4, 0] = np.nan
    tr[5, 1] = -np.inf
    tr[6] = (2.0, 1.0)
    o[7, 0] = np.inf
    d[8, 0] = np.nan
    tr[9, 1] = np.inf
    tr[10] = (-1.0, 4.0)  # t0 < 0 from inside: a_0 = t0 < 0, the step clamps to dt_min
    o[11] = (outer[0, 0] - 0.1 * ext[0], hi0[1], mid[2])  # along x in the plane of level 0's +y face: grazes it (and lies on cell faces of every level)
    d[11] = (1.3 * ext[0], 0.0, 0.0)
    o[12] = outer[1] + 0.2 * ext  # outside, pointing away: misses box K - 1
    d[12] = 0.5 * ext
    d[13] = 0.0  # |d| = 0
    o[14] = mid - np.array([0.0, 0.0, 0.9]) * ext  # axis-parallel through the centre, from outside
    d[14] = (0.0, 0.0, 1.5 * ext[2])
    o[15] = mid - np.array([0.7, 0.6, 0.0]) * ext  # one zero component, from outside box K - 1
    d[15] = (0.9 * ext[0], 0.8 * ext[1], 0.0)
    return o.astype(np.float32), d.astype(np.float32), tr.astype(np.float32), kinds


def mask_points(S, seed, aabbs):
    """S points over the outermost box grown by 10 %, a third of them drawn inside level 0 grown by 10 %, the corners and face centres of
    every level first; and their steps, log-uniform across every level's edge with a few set exactly to an edge, zero, NaN and inf"""
    K = aabbs.shape[0]
    rng = np.random.default_rng(seed)
    sp = np.concatenate([OC.special_points(aabbs[c].reshape(2, 3))[0] for c in range(K)])
    n = S - sp.shape[0]
    pts = OC.to_world(rng.random((n, 3)) * 1.2 - 0.1, aabbs[K - 1].reshape(2, 3))
    pts[::3] = OC.to_world(rng.random((len(pts[::3]), 3)) * 1.2 - 0.1, aabbs[0].reshape(2, 3))
    pts = np.concatenate([sp, pts]).astype(np.float32)
    e0 = float((aabbs[0, 3:] - aabbs[0, :3]).min())
    delta = (e0 / 64 * 2.0 ** rng.uniform(0, K + 7, S)).astype(np.float32)
    return pts, delta


# ---------------------------------------------------------------------------------------------------
# the rules in numpy float32, operation by operation
# ---------------------------------------------------------------------------------------------------
def f32_edges(aabbs, G):
    ext = (aabbs[:, 3:] - aabbs[:, :3]).astype(np.float32)
    return (ext / np.float32(G)).astype(np.float32).min(1)


def f32_cells(p, box, G):
    """(has (n,), cell (n,3)) by the GRID rule of include/lab4d_occgrid.h in float32"""
    lo, hi = box[:3], box[3:]
    ext = (hi - lo).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        x01 = ((p - lo).astype(np.float32) / ext).astype(np.float32)
        has = ((x01 >= 0) & (x01 <= 1)).all(-1) & bool((ext > 0).all())
        q = (x01 * np.float32(G)).astype(np.float32)
        cell = np.minimum(np.nan_to_num(q, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64), G - 1)
    return has, np.where(has[:, None], cell, 0)


def f32_level_rule(p, delta, aabbs, occ, G):
    """LEVEL in float32: (kept (n,), level (n,) with -1 where there is no cell)"""
    K, n = aabbs.shape[0], p.shape[0]
    has, cell = zip(*[f32_cells(p, aabbs[c], G) for c in range(K)])
    has, cell = np.stack(has), np.stack(cell)  # (K, n), (K, n, 3)
    c_pos = np.where(has.any(0), has.argmax(0), -1)
    edges = f32_edges(aabbs, G)
    with np.errstate(invalid="ignore"):
        fits = delta[None, :] <= edges[:, None]
    c_step = np.where(fits.any(0), fits.argmax(0), K - 1)
    level = np.where(c_pos >= 0, np.maximum(c_pos, c_step), -1)
    lv = np.maximum(level, 0)
    rows = np.arange(n)
    cl = cell[lv, rows]
    kept = (level >= 0) & has[lv, rows] & occ[lv, cl[:, 0], cl[:, 1], cl[:, 2]]
    return kept, level


def f32_clip(o, d, tr, box):
    """REJECT and CLIP of lab4d_amd/csrc/ray_math.hpp in float32: (hit (R,), t_in, t_out, len)"""
    f = np.float32
    lo, hi = box[:3], box[3:]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t0, t1 = tr[:, 0], tr[:, 1]
        ext = (hi - lo).astype(f)
        ok = np.isfinite(t0) & np.isfinite(t1) & (t0 <= t1) & np.isfinite(o).all(1) & np.isfinite(d).all(1) & bool((np.isfinite(ext) & (ext > 0)).all())
        ln = np.sqrt(((d[:, 0] * d[:, 0]).astype(f) + (d[:, 1] * d[:, 1]).astype(f)).astype(f) + (d[:, 2] * d[:, 2]).astype(f)).astype(f)
        ok &= ln > 0
        tmin, tmax = t0.copy(), t1.copy()
        miss = np.zeros(o.shape[0], bool)
        for a in range(3):
            o01 = ((o[:, a] - lo[a]).astype(f) / ext[a]).astype(f)
            d01 = (d[:, a] / ext[a]).astype(f)
            ok &= np.isfinite(o01)
            inv = np.where(d01 != 0, (f(1) / np.where(d01 != 0, d01, f(1))).astype(f), f(0))
            par = ~((d01 != 0) & np.isfinite(inv))
            miss |= par & ~((o01 >= 0) & (o01 <= 1))
            ta, tb = ((f(0) - o01).astype(f) * inv).astype(f), ((f(1) - o01).astype(f) * inv).astype(f)
            tn, tf = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            tmin = np.where(~par & (tn > tmin), tn, tmin)
            tmax = np.where(~par & (tf < tmax), tf, tmax)
        hit = ok & ~miss & (tmin <= tmax)
    return hit, tmin.astype(f), tmax.astype(f), ln


def f32_candidates(o, d, tr, aabbs, cone, dt_min, dt_max, k_max):
    """STEPS in float32: dict of (R, k_max) arrays a (interval start), s, t, delta, cand (candidate k exists), p (R, k_max, 3), and len, hit,
    t_in, t_out per ray"""
    f = np.float32
    o, d, tr = _c(o, f), _c(d, f), _c(tr, f)
    R, K = o.shape[0], aabbs.shape[0]
    hit, t_in, t_out, ln = f32_clip(o, d, tr, aabbs[K - 1])
    cone, dt_min, dt_max = f(cone), f(dt_min), f(dt_max)
    A, S, T, D = (np.zeros((R, k_max), f) for _ in range(4))
    P, cand = np.zeros((R, k_max, 3), f), np.zeros((R, k_max), bool)
    a, alive = np.where(hit, t_in, f(0)).astype(f), hit.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(k_max):
            x = (a * cone).astype(f)
            s = np.where(x > dt_min, x, dt_min).astype(f)
            s = np.where(s < dt_max, s, dt_max).astype(f)
            t = (a + (f(0.5) * s).astype(f)).astype(f)
            alive = alive & (t <= t_out)
            A[:, k], S[:, k], T[:, k], cand[:, k] = a, s, t, alive
            D[:, k] = (s * ln).astype(f)
            P[:, k] = (o + (t[:, None] * d).astype(f)).astype(f)
            a = (a + s).astype(f)
    return {"a": A, "s": S, "t": T, "delta": D, "p": P, "cand": cand, "len": ln, "hit": hit, "t_in": t_in, "t_out": t_out}


def f32_march(o, d, tr, aabbs, occ, G, cone, dt_min, dt_max, k_max, cap=None, tail=0):
    """The whole contract in numpy float32: host_march's dict (with `kept` (R, k_max) and the candidates `c` on top)"""
    f = np.float32
    c = f32_candidates(o, d, tr, aabbs, cone, dt_min, dt_max, k_max)
    R, K = c["t"].shape[0], aabbs.shape[0]
    kept, level = f32_level_rule(c["p"].reshape(-1, 3), c["delta"].reshape(-1), aabbs, occ, G)
    kept, level = kept.reshape(R, k_max) & c["cand"], level.reshape(R, k_max)
    count = kept.sum(1).astype(np.int32)
    start = (np.cumsum(count) - count).astype(np.int32)
    total = int(count.sum())
    if cap is None:
        cap = total
    n = min(total, cap)
    r, k = np.nonzero(kept)  # ray order, ascending k
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where((c["len"] > 0)[:, None], (_c(d, f) / np.where(c["len"] > 0, c["len"], f(1))[:, None]).astype(f), f(0))
    outer = aabbs[K - 1]
    park = (outer[3:] + (outer[3:] - outer[:3]).astype(f)).astype(f)
    out = {"t": np.full(cap + tail, np.nan, f), "steps": np.full(cap + tail, np.nan, f), "deltas": np.full(cap + tail, np.nan, f),
           "xyz": np.full((cap + tail, 3), np.nan, f), "dirs": np.full((cap + tail, 3), np.nan, f), "ray_idx": np.full(cap + tail, -7, np.int32),
           "level": np.full(cap + tail, -7, np.int32)}
    out["t"][:n], out["steps"][:n], out["deltas"][:n] = c["t"][r, k][:n], c["s"][r, k][:n], c["delta"][r, k][:n]
    out["xyz"][:n], out["dirs"][:n], out["ray_idx"][:n], out["level"][:n] = c["p"][r, k][:n], u[r][:n], r[:n], level[r, k][:n]
    out["t"][n:cap], out["steps"][n:cap], out["deltas"][n:cap], out["xyz"][n:cap], out["dirs"][n:cap] = 0, 0, 0, park, (0, 0, 1)
    out["ray_idx"][n:cap], out["level"][n:cap] = -1, -1
    out.update(ray_start=start, ray_count=np.clip(cap - start.astype(np.int64), 0, count).astype(np.int32), total=total, overflow=total > cap, count=count,
               R=R, cap=cap, kept=kept, c=c)
    return out


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, ref, what):
    """two march dicts (the twin's, numpy's, or the kernels' brought to numpy) equal to the word: the counts, total, overflow, every row, the
    parked rows, and the sentinels behind the cap where both sides allocated a tail"""
    assert got["total"] == ref["total"] and got["overflow"] == ref["overflow"], (what, got["total"], ref["total"])
    for k in ("ray_count", "ray_start", "ray_idx", "level"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k)
    for k in FIELDS:
        a, b = words(got[k]), words(ref[k])
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))


# ---------------------------------------------------------------------------------------------------
# the kept set in float64
# ---------------------------------------------------------------------------------------------------
def f64_classification(o, d, c, aabbs, occ, G):
    """The LEVEL rule on the SAME candidates (t_k and s_k as float32 formed them) with the points, the steps' world lengths, the edges, the
    levels and the cells in float64: (keep (R,K), level (R,K), clear (R,K)); clear = x01 * G is farther than OC.MARGIN from an integer on
    all axes at the level used, and delta is farther than a relative 1e-5 from every edge_c"""
    K = aabbs.shape[0]
    R, kk = c["t"].shape
    o64, d64 = np.nan_to_num(np.asarray(o, np.float64)), np.nan_to_num(np.asarray(d, np.float64))
    p = (o64[:, None, :] + c["t"].astype(np.float64)[:, :, None] * d64[:, None, :]).reshape(-1, 3)
    delta = (c["s"].astype(np.float64) * np.linalg.norm(d64, axis=1)[:, None]).reshape(-1)
    b = aabbs.astype(np.float64)
    x01 = np.stack([(p - b[cc, :3]) / (b[cc, 3:] - b[cc, :3]) for cc in range(K)])  # (K, n, 3)
    has = ((x01 >= 0) & (x01 <= 1)).all(-1)
    edges = ((b[:, 3:] - b[:, :3]) / G).min(1)
    fits = delta[None, :] <= edges[:, None]
    c_pos = np.where(has.any(0), has.argmax(0), -1)
    c_step = np.where(fits.any(0), fits.argmax(0), K - 1)
    level = np.where(c_pos >= 0, np.maximum(c_pos, c_step), -1)
    lv, rows = np.maximum(level, 0), np.arange(p.shape[0])
    q = x01[lv, rows] * G
    cell = np.clip(np.floor(q), 0, G - 1).astype(np.int64)
    keep = (level >= 0) & has[lv, rows] & occ[lv, cell[:, 0], cell[:, 1], cell[:, 2]]
    clear = (np.abs(q - np.round(q)) > OC.MARGIN).all(-1) & (np.abs(delta[None, :] - edges[:, None]) > 1e-5 * edges[:, None]).all(0)
    return keep.reshape(R, kk), level.reshape(R, kk), clear.reshape(R, kk)


def generic_rays(n, seed, aabbs):
    """rays for the float64 comparison: a third from outside box K - 1 through a random point of it, a third from inside it, a third from
    inside level 0; directions of length 0.5 .. 2 outer box edges, no component exactly zero; t0 in [0, 0.2], t1 in [3, 6]"""
    K = aabbs.shape[0]
    rng = np.random.default_rng(seed)
    outer, inner = aabbs[K - 1].reshape(2, 3), aabbs[0].reshape(2, 3)
    o, d, tr = outside_rays(n, rng, outer)
    third = n // 3
    o[third:2 * third] = OC.to_world(rng.uniform(0.02, 0.98, (third, 3)), outer)
    o[2 * third:] = OC.to_world(rng.uniform(0.02, 0.98, (n - 2 * third, 3)), inner)
    return o, d, tr


def outside_rays(n, rng, box):
    u = rng.standard_normal((n, 3))
    o = 0.5 + u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))
    d = (rng.uniform(0.02, 0.98, (n, 3)) - o) * rng.uniform(0.5, 2.0, (n, 1))
    lo, ext = box[0].astype(np.float64), box[1].astype(np.float64) - box[0]
    t = np.stack([rng.uniform(0.0, 0.2, n), rng.uniform(3.0, 6.0, n)], 1)
    return (lo + o * ext).astype(np.float32), (d * ext).astype(np.float32), t.astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# the cascade's update rule in numpy
# ---------------------------------------------------------------------------------------------------
def parent_index(G):
    """cell i of level c - 1 along an axis lies in cell (i + G/2) // 2 of level c (both boxes share their centre, the cells double)"""
    return (np.arange(G) + G // 2) // 2


def np_propagate(density, K, G):
    """(K, G^3) float32 -> (K, G, G, G): NaN and negative as 0, +inf as the largest finite value (an ema of +inf means "nothing known yet"
    to UPDATE, which would forget the cell's history at the next update, on one level and not on the other); level c raised to the maximum
    over the children of each of its cells"""
    with np.errstate(invalid="ignore"):
        d = np.where(density > 0, np.minimum(density, F32_MAX), np.float32(0)).astype(np.float32).reshape(K, G, G, G)
    j = parent_index(G)
    I, J, L = np.meshgrid(j, j, j, indexing="ij")
    for c in range(1, K):
        np.maximum.at(d[c], (I, J, L), d[c - 1])
    return d


def np_cascade_new(K, G):
    return np.full((K, G ** 3), np.inf, np.float32)


def np_cascade_update(ema, density, K, G, decay, thresh):
    """in place on ema (K, G^3): UPDATE of include/lab4d_occgrid.h per level on the propagated density; returns the bits as (K, G, G, G) bool"""
    d = np_propagate(density, K, G).reshape(K, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (ema * np.float32(decay)).astype(np.float32)
        ema[:] = np.where(ema > F32_MAX, d, np.where(prod > d, prod, d))
    return (ema > np.float32(thresh)).reshape(K, G, G, G)


def parents_hold(occ):
    """every set bit of level c - 1 has its parent bit set at level c"""
    K, G = occ.shape[0], occ.shape[1]
    j = parent_index(G)
    I, J, L = np.meshgrid(j, j, j, indexing="ij")
    return all(bool(occ[c][I, J, L][occ[c - 1]].all()) for c in range(1, K))


def cascade_density(K, G, seed):
    return np.stack([OC.density_volume(G, seed + c) for c in range(K)])
