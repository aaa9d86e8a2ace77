"""Shared by tests/test_occgrid_host.py (CPU twin against numpy in float64) and tests/test_gpu_zzzzoccgrid.py (kernels against the twin,
bit for bit): the host harness of the occupancy grid (tests/host_harness/occgrid_host.cpp over lab4d_amd/csrc/occgrid_math.hpp), the
test inputs, and the rules of include/lab4d_occgrid.h restated in numpy float64 (vectorised; shares no code with the header)."""
import os

import numpy as np

import host_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a box that is neither cubic nor centred, so that the three axes scale differently
AABB = np.array([[-0.12, -0.10, -0.15], [0.12, 0.14, 0.09]], np.float32)
MARGIN = 1e-4  # of a cell edge: where the float32 rule and the float64 rule may put a point into different cells


def build_host():
    return host_twin.load("occgrid")


def n_words(G):
    return (G ** 3 + 31) // 32


def host_init(lib, G):
    """(ema (G^3,) f32, bits (words,) u32, n_occupied int) of a new grid"""
    ema, bits, n = np.empty(G ** 3, np.float32), np.empty(n_words(G), np.uint32), np.zeros(1, np.int32)
    lib.occgrid_host_init(ema.ctypes.data, bits.ctypes.data, n.ctypes.data, G)
    return ema, bits, int(n[0])


def host_update(lib, density, ema, bits, G, decay, thresh):
    """in place on ema / bits; returns n_occupied"""
    density = np.ascontiguousarray(density, np.float32).reshape(-1)
    assert density.size == G ** 3 and ema.dtype == np.float32 and bits.dtype == np.uint32
    n = np.zeros(1, np.int32)
    lib.occgrid_host_update(density.ctypes.data, ema.ctypes.data, bits.ctypes.data, n.ctypes.data, G, decay, thresh)
    return int(n[0])


def host_mask(lib, xyz, aabb, bits, G):
    xyz, aabb = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(aabb, np.float32)
    out = np.empty(xyz.shape[0], np.uint8)
    lib.occgrid_host_mask(xyz.ctypes.data, aabb.ctypes.data, bits.ctypes.data, G, xyz.shape[0], out.ctypes.data)
    return out


def host_ray_span(lib, origin, direction, t_range, aabb, bits, G):
    """(t_span (R,2) f32, hit (R,) u8, steps (R,) i32)"""
    origin, direction, t_range = (np.ascontiguousarray(a, np.float32) for a in (origin, direction, t_range))
    aabb = np.ascontiguousarray(aabb, np.float32)
    R = origin.shape[0]
    span, hit, steps = np.empty((R, 2), np.float32), np.empty(R, np.uint8), np.empty(R, np.int32)
    lib.occgrid_host_ray_span(origin.ctypes.data, direction.ctypes.data, t_range.ctypes.data, aabb.ctypes.data, bits.ctypes.data, G, R, span.ctypes.data,
                              hit.ctypes.data, steps.ctypes.data)
    return span, hit, steps


# ---------------------------------------------------------------------------------------------------
# bit layout, restated
# ---------------------------------------------------------------------------------------------------
def pack(occ):
    """(G,G,G) bool, x slowest -> uint32 words: cell idx is bit idx & 31 of word idx >> 5, padding zero"""
    flat = np.asarray(occ, bool).reshape(-1)
    words = np.zeros((flat.size + 31) // 32, np.uint32)
    idx = np.nonzero(flat)[0]
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def unpack(words, G):
    idx = np.arange(G ** 3)
    return ((words[idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool).reshape(G, G, G)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def random_occupancy(G, seed, density=0.05):
    return np.random.default_rng(seed).random((G, G, G)) < density


def sphere_occupancy(G, r=0.3):
    """cells whose centre lies within r (in x01 units) of the box centre"""
    ax = (np.arange(G) + 0.5) / G - 0.5
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return X * X + Y * Y + Z * Z < r * r


def density_volume(G, seed):
    """random densities around the default threshold, with the values the update rule singles out: NaN, negative, zero, +inf"""
    rng = np.random.default_rng(seed)
    d = (rng.random(G ** 3) * 0.04).astype(np.float32)
    k = rng.permutation(G ** 3)
    q = max(1, G ** 3 // 16)
    d[k[:q]] = np.nan
    d[k[q:2 * q]] = -1.0
    d[k[2 * q:3 * q]] = 0.0
    d[k[3 * q]] = np.inf
    return d


def to_world(x01, aabb=AABB):
    lo, hi = aabb[0].astype(np.float64), aabb[1].astype(np.float64)
    return (lo + np.asarray(x01, np.float64) * (hi - lo)).astype(np.float32)


def special_points(aabb=AABB):
    """(points (n,3) f32, in_box (n,) bool): the 8 corners (x01 exactly 0 / 1), face centres, a point 1e-6 of the box outside each face, NaN"""
    lo, hi = aabb[0], aabb[1]
    mid = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    pts, inb = [], []
    for c in range(8):
        pts.append([(hi if (c >> a) & 1 else lo)[a] for a in range(3)])
        inb.append(True)
    for a in range(3):
        for side, sign in ((lo, -1), (hi, 1)):
            p = mid.copy()
            p[a] = side[a]
            pts.append(p.copy())
            inb.append(True)
            p[a] = side[a] + np.float32(sign * 1e-6) * (hi[a] - lo[a])  # x01 = -1e-6 / 1 + 1e-6: eight float32 steps past the face
            pts.append(p.copy())
            inb.append(False)
        p = mid.copy()
        p[a] = np.nan
        pts.append(p)
        inb.append(False)
    return np.array(pts, np.float32), np.array(inb)


def mask_points(S, seed, aabb=AABB):
    """S points: the special ones first, then uniform over the box grown by 10 % on every side"""
    sp, _ = special_points(aabb)
    rng = np.random.default_rng(seed)
    rnd = to_world(rng.random((S - sp.shape[0], 3)) * 1.2 - 0.1, aabb)
    return np.concatenate([sp, rnd], 0)


N_RAYS = 1025


def rays(seed, aabb=AABB):
    """(origin (1025,3), dir (1025,3), t_range (1025,2)) float32 world rays, and a dict name -> slice of the kinds.  Built in x01 space (box =
    [0,1]^3), origins within 1.1 box edges of the centre, directions of length 0.5 .. 2 (t is NOT a distance)."""
    rng = np.random.default_rng(seed)

    def unit(n):
        v = rng.standard_normal((n, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def outside(n):
        return 0.5 + unit(n) * rng.uniform(0.9, 1.1, (n, 1))

    def inside(n):
        return rng.uniform(0.02, 0.98, (n, 3))

    O, D, T, kinds = [], [], [], {}

    def add(name, o, d, t0, t1):
        kinds[name] = slice(sum(len(x) for x in O), sum(len(x) for x in O) + len(o))
        O.append(o), D.append(d), T.append(np.stack([np.broadcast_to(t0, (len(o),)), np.broadcast_to(t1, (len(o),))], 1))

    # random: from outside through a random point of the box, far enough to leave it again
    n = 398
    o, tgt = outside(n), inside(n)
    d = (tgt - o) * rng.uniform(0.5, 2.0, (n, 1))
    add("random", o, d, rng.uniform(0.0, 0.2, n), rng.uniform(3.0, 6.0, n))
    # the two space diagonals through cell corners (o01 = -1 / 2, d01 = +-1 exactly in float32 as well): every step is a three-way tie
    add("diagonal", np.array([[-1.0] * 3, [2.0] * 3]), np.array([[1.0] * 3, [-1.0] * 3]), 0.0, 4.0)
    # axis-parallel: one and two zero components, both signs; a third of them beside the box (zero-component slab never satisfied)
    n = 150
    o, d = inside(n), np.zeros((n, 3))
    for i in range(n):
        axes = rng.permutation(3)[:1 if i % 2 else 2]  # the moving axes
        for a in axes:
            s = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 2.0)
            d[i, a] = s
            o[i, a] = -0.4 if s > 0 else 1.4
        if i % 3 == 0:
            still = [a for a in range(3) if a not in axes]
            o[i, still[0]] = rng.choice([-0.2, 1.2])
    add("axis", o, d, 0.0, rng.uniform(2.0, 5.0, n))
    # origin inside the box
    n = 150
    add("inside", inside(n), unit(n) * rng.uniform(0.5, 2.0, (n, 1)), rng.uniform(0.0, 0.1, n), rng.uniform(2.0, 4.0, n))
    # miss the box: pointing away from it, or ending before it
    n = 100
    o = outside(n)
    d = (o - 0.5) * rng.uniform(0.5, 2.0, (n, 1)) + unit(n) * 0.2
    d[n // 2:] = (inside(n - n // 2) - o[n // 2:])
    t1 = np.where(np.arange(n) < n // 2, 4.0, 0.05)
    add("miss", o, d, 0.0, t1)
    # t1 ends inside the box: d = target - origin, t1 < 1
    n = 125
    o = outside(n)
    add("t1_inside", o, inside(n) - o, 0.0, rng.uniform(0.7, 0.99, n))
    # all three components negative
    n = 100
    o = 0.5 + np.abs(unit(n)) * rng.uniform(0.9, 1.1, (n, 1))
    d = -(np.abs(o - inside(n)) + 0.05) * rng.uniform(0.5, 2.0, (n, 1))
    add("negative", o, d, 0.0, rng.uniform(3.0, 6.0, n))
    o, d, t = np.concatenate(O), np.concatenate(D), np.concatenate(T)
    assert o.shape[0] == N_RAYS
    lo, ext = aabb[0].astype(np.float64), aabb[1].astype(np.float64) - aabb[0]
    return (lo + o * ext).astype(np.float32), (d * ext).astype(np.float32), t.astype(np.float32), kinds


# ---------------------------------------------------------------------------------------------------
# the rules in float64
# ---------------------------------------------------------------------------------------------------
def x01_f64(p, aabb=AABB):
    lo, hi = aabb[0].astype(np.float64), aabb[1].astype(np.float64)
    return (np.asarray(p, np.float64) - lo) / (hi - lo)


def ref_cells(x01, G):
    """(has_cell (n,), cell (n,3) int, clear (n,)): the float64 cell rule; clear = every coordinate farther than MARGIN cell edges from
    every cell face (the box faces included)"""
    with np.errstate(invalid="ignore"):
        has = ((x01 >= 0) & (x01 <= 1)).all(-1)
        q = x01 * G
        cell = np.clip(np.floor(np.nan_to_num(q)), 0, G - 1).astype(np.int64)
        clear = (np.abs(q - np.round(q)) > MARGIN).all(-1)
    return has, cell, clear


def ref_mask(points, occ, G, aabb=AABB):
    has, cell, clear = ref_cells(x01_f64(points, aabb), G)
    return has & occ[cell[:, 0], cell[:, 1], cell[:, 2]], clear


def ref_ray_samples(origin, direction, t_range, occ, G, n_t=4096, aabb=AABB, chunk=64):
    """For every ray, n_t evenly spaced t in [t0, t1] in float64: (t (R,n_t), good (R,n_t), n_margin): good = the float64 point lies in an
    occupied cell, clear of every cell face; n_margin = the number of (ray, t) pairs in an occupied cell that the face margin leaves out."""
    R = origin.shape[0]
    z = np.linspace(0.0, 1.0, n_t)
    t = t_range[:, :1].astype(np.float64) * (1 - z) + t_range[:, 1:].astype(np.float64) * z
    good = np.zeros((R, n_t), bool)
    n_margin = 0
    for r0 in range(0, R, chunk):
        sl = slice(r0, r0 + chunk)
        p = origin[sl, None, :].astype(np.float64) + t[sl, :, None] * direction[sl, None, :].astype(np.float64)
        has, cell, clear = ref_cells(x01_f64(p.reshape(-1, 3), aabb), G)
        in_occ = has & occ[cell[:, 0], cell[:, 1], cell[:, 2]]
        good[sl] = (in_occ & clear).reshape(-1, n_t)
        n_margin += int((in_occ & ~clear).sum())
    return t, good, n_margin


def ref_walk(origin, direction, t_range, occ, G, aabb=AABB):
    """The span rules in float64, vectorised over the rays: (entry (R,3G), exit (R,3G), occupied (R,3G)) of the cells each ray visits (slots
    behind a ray's last cell: occupied = False), entry / exit clipped to the ray's part inside the box and [t0, t1]."""
    ext = aabb[1].astype(np.float64) - aabb[0]
    o = x01_f64(origin, aabb)
    d = direction.astype(np.float64) / ext
    R = o.shape[0]
    tmin, tmax = t_range[:, 0].astype(np.float64).copy(), t_range[:, 1].astype(np.float64).copy()
    alive = tmin <= tmax
    mv = d != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(mv, 1.0 / np.where(mv, d, 1.0), 0.0)
    for a in range(3):
        ta, tb = (0 - o[:, a]) * inv[:, a], (1 - o[:, a]) * inv[:, a]
        tmin = np.where(mv[:, a], np.maximum(tmin, np.minimum(ta, tb)), tmin)
        tmax = np.where(mv[:, a], np.minimum(tmax, np.maximum(ta, tb)), tmax)
        alive &= mv[:, a] | ((o[:, a] >= 0) & (o[:, a] <= 1))
    alive &= tmin <= tmax
    p = o + np.where(alive, tmin, 0.0)[:, None] * d
    c = np.clip(np.floor(p * G), 0, G - 1).astype(np.int64)
    up = d > 0
    n = 3 * G
    entry, exit_, occd = np.zeros((R, n)), np.zeros((R, n)), np.zeros((R, n), bool)
    t_cur = tmin.copy()
    rows = np.arange(R)
    for s in range(n):
        ex = np.where(mv, ((c + up) / G - o) * inv, np.inf)
        ax = np.argmin(ex, 1)  # ties: the lowest index
        t_exit = np.maximum(np.minimum(ex[rows, ax], np.inf), t_cur)
        t_exit = np.where(mv.any(1), t_exit, tmax)
        entry[:, s], exit_[:, s] = t_cur, np.minimum(t_exit, tmax)
        occd[:, s] = alive & occ[c[:, 0], c[:, 1], c[:, 2]]
        alive = alive & mv.any(1) & (t_exit < tmax)
        c[rows, ax] += np.where(up[rows, ax], 1, -1)
        alive &= (c[rows, ax] >= 0) & (c[rows, ax] < G)
        c = np.clip(c, 0, G - 1)
        t_cur = np.where(alive, t_exit, t_cur)
    assert not alive.any(), "the float64 walk needs more than 3 G cells"
    return entry, exit_, occd


def cell_diagonal_t(direction, G, aabb=AABB):
    """length of a cell's diagonal in the ray's own parameter: sqrt(3) / G in x01 space over |d01|"""
    d01 = direction.astype(np.float64) / (aabb[1].astype(np.float64) - aabb[0])
    return np.sqrt(3.0) / G / np.linalg.norm(d01, axis=1)
