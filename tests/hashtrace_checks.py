"""Shared by tests/test_hashtrace_host.py (CPU twin) and tests/test_gpu_zzzzzzzzzzhashtrace.py (kernel): the host harness of the sphere tracer
(tests/host_harness/hashtrace/hashtrace_host.cpp over lab4d_amd/csrc/hashtrace_math.hpp), the test fields, the ray sets and the truth: the
field in float64 over oracle/hashgrid_oracle.py on 4,096 points of the clipped ray, the first sign change bisected to 1e-12.  Nothing of the
code under test enters the truth.  Everything built here is cached and shared between the two suites: never modified.

FIELDS  (a) analytic: feature 0 of level 0 (dense) holds a shape's exact signed distance at that level's vertices in world units, every other
        table entry is zero, W1 rows 0 / 1 = +e_0 / -e_0, w2 = [1, -1, 0, ...], biases zero: the field IS the tri-linear interpolant of the
        shape (relu(s) - relu(-s) = s), with |grad| close to 1.  "sphere": radius 0.08 at the centre of the default 0.24 box; "two": radii 0.05
        and 0.04; "sphere4": the sphere at F = 4.
        (b) "random": hashfield.make_weights(0, sdf_bias=...) on a small table (x 1e3, as tests/hashsdf_checks.py does, so that the field
        varies), the bias set so that the median of the field over the box is 0.  For invariants only.
RAYS    origins 0.5 from the box centre, `dir` of length 0.5 .. 2, t_range = [0, 1 / len].  HIT: aimed at a point within 0.8 r of a sphere's
        centre (impact parameter <= 0.8 r: incidence cosine >= 0.6).  MISS: aimed at a point of the box, impact parameter >= 1.3 r to every
        sphere.  Both sets are CHOSEN so that every ray's impact parameter to every sphere lies outside (0.8 r, 1.3 r): no ray grazes, and the
        comparisons leave out none."""
import functools
import os

import numpy as np
import torch

import host_twin
from oracle import hashgrid_oracle as HO

TWIN = "hashtrace/hashtrace"  # tests/host_harness/hashtrace/hashtrace_host.cpp: a folder of its own (tests/test_host_twin.py pins the census of the twins beside it)
EPS = 1e-4
T_BOUND = 5.0  # |t_hit - t_ref| * len <= T_BOUND * eps: both satisfy |sdf| <= eps where the directional derivative is >= 0.6 x ~0.9
MISS, CONVERGED, BRACKETED, STARTS_INSIDE, OUT_OF_STEPS = range(5)
SHAPES = {"sphere": ([(0.0, 0.0, 0.0)], [0.08]), "two": ([(-0.05, -0.01, 0.0), (0.06, 0.02, 0.01)], [0.05, 0.04])}
CONFIGS = {2: {"L": 16, "F": 2, "n_min": 16, "n_max": 256, "log2_T": 13}, 4: {"L": 8, "F": 4, "n_min": 16, "n_max": 256, "log2_T": 13},
           "random": {"L": 16, "F": 2, "n_min": 4, "n_max": 32, "log2_T": 12}}
DEFAULTS = dict(eps=EPS, step_scale=1.0, min_step=EPS, max_steps=128, n_bisect=8)


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def res_list(cfg):
    return HO.level_resolutions(cfg["L"], cfg["n_min"], cfg["n_max"])


# ---------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------
def shape_of(name):
    centres, radii = SHAPES["sphere" if name == "sphere4" else name]
    return np.array(centres, np.float64), np.array(radii, np.float64)


@functools.lru_cache(None)
def field(name):
    """P (float32, CPU), cfg of the fields above"""
    from lab4d_amd import hashfield
    if name == "random":
        P, cfg = hashfield.make_weights(0, cfg=CONFIGS["random"], sdf_bias=0.0)
        P["hash.table"] = P["hash.table"] * 1e3
        g = torch.Generator().manual_seed(5)
        pts = P["aabb"][0] + torch.rand(4096, 3, generator=g) * (P["aabb"][1] - P["aabb"][0])
        P["hash.geo.2.bias"][0] = -float(sdf64(P, cfg, pts.double()).median())
        return P, cfg
    P, cfg = hashfield.make_weights(0, cfg=CONFIGS[4 if name == "sphere4" else 2])
    centres, radii = shape_of(name)
    r0 = res_list(cfg)[0]
    assert (r0 + 1) ** 3 <= 1 << cfg["log2_T"]  # level 0 is dense
    lo, hi = P["aabb"][0].double().numpy(), P["aabb"][1].double().numpy()
    ax = [lo[a] + (hi[a] - lo[a]) * np.arange(r0 + 1) / r0 for a in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")  # vertex (ix, iy, iz) sits at ix + n (iy + n iz)
    pts = np.stack([X, Y, Z], -1)
    dist = np.min(np.linalg.norm(pts[..., None, :] - centres, axis=-1) - radii, -1)
    table = torch.zeros_like(P["hash.table"])
    table[0, :(r0 + 1) ** 3, 0] = torch.from_numpy(dist.transpose(2, 1, 0).reshape(-1)).float()
    P["hash.table"] = table
    W1, w2 = torch.zeros(64, 32), torch.zeros(16, 64)
    W1[0, 0], W1[1, 0], w2[0, 0], w2[0, 1] = 1.0, -1.0, 1.0, -1.0
    P["hash.geo.0.weight"], P["hash.geo.0.bias"] = W1, torch.zeros(64)
    P["hash.geo.2.weight"], P["hash.geo.2.bias"] = w2, torch.zeros(16)
    return P, cfg


def sdf64(P, cfg, pts, with_grad=False):
    """the field in float64 at world points pts (S,3) float64, x01 clamped into the box as the tracer's rule says; with_grad: also d sdf / d pts"""
    pts = pts.double().clone().requires_grad_(with_grad)
    lo, hi = P["aabb"][0].double(), P["aabb"][1].double()
    x01 = ((pts - lo) / (hi - lo)).clamp(0.0, 1.0)
    enc = HO.hash_encode(x01, P["hash.table"].double(), res_list(cfg), cfg["log2_T"])
    h = torch.relu(enc @ P["hash.geo.0.weight"].double().T + P["hash.geo.0.bias"].double())
    s = h @ P["hash.geo.2.weight"][0].double() + P["hash.geo.2.bias"][0].double()
    if not with_grad:
        return s.detach()
    g, = torch.autograd.grad(s.sum(), pts)
    return s.detach(), g


# ---------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------
def impact(o, d, centres):
    """(R, K) float64: distance of every sphere centre from the ray's line"""
    o, d = o.astype(np.float64), d.astype(np.float64)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    w = centres[None] - o[:, None]
    return np.linalg.norm(w - (w * u[:, None]).sum(-1, keepdims=True) * u[:, None], axis=-1)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(None)
def rays(name, kind, n, seed=0):
    """origin, dir (n,3), t_range (n,2) float32 of the HIT / MISS / INSIDE set of an analytic field, or GENERIC rays through the box"""
    rng = np.random.default_rng(1000 * seed + {"hit": 1, "miss": 2, "inside": 3, "generic": 4}[kind])
    centres, radii = shape_of(name) if name != "random" else (np.zeros((1, 3)), np.array([0.08]))
    m = 8 * n + 64
    k = rng.integers(0, len(radii), m)
    ball = _unit(rng, m) * rng.random((m, 1)) ** (1 / 3)
    if kind == "inside":
        o = centres[k] + 0.5 * radii[k, None] * ball
        d = _unit(rng, m) * rng.uniform(0.5, 2.0, (m, 1))
        keep = np.ones(m, bool)
    else:
        o = 0.5 * _unit(rng, m)
        target = centres[k] + 0.8 * radii[k, None] * ball if kind == "hit" else rng.uniform(-0.11, 0.11, (m, 3))
        d = target - o
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (m, 1))
        o, d = o.astype(np.float32), d.astype(np.float32)
        b = impact(o, d, centres)
        if kind == "hit":
            keep = ((b <= 0.8 * radii) | (b >= 1.3 * radii)).all(1) & (b <= 0.8 * radii).any(1)
        elif kind == "miss":
            keep = (b >= 1.3 * radii).all(1)
        else:
            keep = np.ones(m, bool)
    o, d = o[keep][:n].astype(np.float32), d[keep][:n].astype(np.float32)
    assert o.shape[0] == n, (kind, int(keep.sum()))
    ln = np.linalg.norm(d.astype(np.float64), axis=1)
    tr = np.stack([np.zeros(n), 1.0 / ln], 1).astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(tr)


def clip64(o, d, tr, P):
    """the slab test in float64: t_enter, t_exit (R,), nonempty (R,) bool (for finite rays with a non-zero direction)"""
    lo, hi = P["aabb"][0].double().numpy(), P["aabb"][1].double().numpy()
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - o) / d, (hi - o) / d
    par = d == 0
    tn = np.where(par, -np.inf, np.minimum(ta, tb))
    tf = np.where(par, np.inf, np.maximum(ta, tb))
    inside = (~par | ((o >= lo) & (o <= hi))).all(1)
    t_in, t_out = np.maximum(tn.max(1), tr[:, 0]), np.minimum(tf.min(1), tr[:, 1])
    return t_in, t_out, inside & (t_in <= t_out)


@functools.lru_cache(None)
def truth(name, kind, n, seed=0, samples=4096):
    """dict: t_enter, t_exit (float64 slab), kind (n,) = 'root' / 'inside' / 'none', t_ref (n,) float64 = the first sign change of the float64
    field over `samples` points of the clipped ray bisected to 1e-12 (nan where there is none)"""
    P, cfg = field(name)
    o, d, tr = rays(name, kind, n, seed)
    t_in, t_out, ok = clip64(o, d, tr, P)
    assert ok.all()
    o64, d64 = torch.from_numpy(o).double(), torch.from_numpy(d).double()
    f = lambda t: sdf64(P, cfg, (o64[:, None] + t[..., None] * d64[:, None]).reshape(-1, 3)).reshape(t.shape)  # noqa: E731
    z = torch.linspace(0, 1, samples, dtype=torch.float64)
    t = torch.from_numpy(t_in)[:, None] * (1 - z) + torch.from_numpy(t_out)[:, None] * z
    v = f(t)
    change = (v[:, :-1] > 0) & (v[:, 1:] <= 0)
    has = change.any(1)
    first = torch.where(has, change.to(torch.int64).argmax(1), torch.zeros(n, dtype=torch.int64))
    a, b = t.gather(1, first[:, None])[:, 0].clone(), t.gather(1, first[:, None] + 1)[:, 0].clone()
    while float((b - a).max()) > 1e-12:
        mid = 0.5 * (a + b)
        pos = f(mid[:, None])[:, 0] > 0
        a, b = torch.where(pos, mid, a), torch.where(pos, b, mid)
    inside = v[:, 0] <= 0
    kinds = np.where(inside.numpy(), "inside", np.where(has.numpy(), "root", "none"))
    t_ref = torch.where(has & ~inside, 0.5 * (a + b), torch.full_like(a, float("nan"))).numpy()
    return {"t_enter": t_in, "t_exit": t_out, "kind": kinds, "t_ref": t_ref}


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32)


def _ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data


def host_clip(lib, o, d, tr, P):
    R = o.shape[0]
    aabb = _np(P["aabb"]).reshape(-1)
    t_clip, ok = np.full((R, 2), 7.0, np.float32), np.full(R, 7, np.uint8)
    lib.hashtrace_host_clip(_ptr(o), _ptr(d), _ptr(tr), aabb.ctypes.data, R, _ptr(t_clip), _ptr(ok))
    return t_clip, ok.astype(bool)


def host_trace(lib, P, cfg, o, d, tr, expect=0, **kw):
    """the twin's t_hit, status, n_eval, sdf_hit (numpy) under DEFAULTS overridden by kw"""
    q = dict(DEFAULTS, **kw)
    o, d, tr = (np.ascontiguousarray(x, np.float32) for x in (o, d, tr))
    R = o.shape[0]
    aabb, table = _np(P["aabb"]).reshape(-1), _np(P["hash.table"])
    res = np.array(res_list(cfg), np.int32)
    W1, b1, w2, b2 = _np(P["hash.geo.0.weight"]), _np(P["hash.geo.0.bias"]), _np(P["hash.geo.2.weight"][0]), _np(P["hash.geo.2.bias"][:1])
    t_hit, sdf_hit = np.full(R, 7.0, np.float32), np.full(R, 7.0, np.float32)
    status, n_eval = np.full(R, -7, np.int32), np.full(R, -7, np.int32)
    rc = lib.hashtrace_host_trace(_ptr(o), _ptr(d), _ptr(tr), aabb.ctypes.data, R, table.ctypes.data, res.ctypes.data, cfg["L"], cfg["log2_T"], cfg["F"],
                                  W1.ctypes.data, b1.ctypes.data, w2.ctypes.data, b2.ctypes.data, q["eps"], q["step_scale"], q["min_step"], q["max_steps"],
                                  q["n_bisect"], _ptr(t_hit), _ptr(status), _ptr(n_eval), _ptr(sdf_hit))
    assert rc == expect, rc
    return t_hit, status, n_eval, sdf_hit


def point_at(o, d, t):
    """o + t d as the tracer forms it: float32, the product and the sum rounded on their own"""
    return (o.astype(np.float32) + (t.astype(np.float32)[:, None] * d.astype(np.float32)).astype(np.float32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# the degenerate rays of the rules
# ---------------------------------------------------------------------------------------------------
def degenerate_rays():
    """origin, dir, t_range (float32) and want (list): the status, 'hit' (1 or 2) or 'rejected' (status 0, n_eval 0, t_hit = t0, sdf_hit = 0) on
    the field "sphere" under DEFAULTS"""
    nan, inf = float("nan"), float("inf")
    rows = [((0, 0, -0.5), (0, 0, 1), (0, 2), "hit"),                    # axis-parallel, through the centre
            ((0.01, -0.5, 0.02), (0, 2, 0), (0, 2), "hit"),              # axis-parallel, |d| = 2
            ((-0.5, 0.02, 0.01), (-1, 0, 0), (-2, 0), "hit"),            # axis-parallel, going down, negative t
            ((0, 0, -0.5), (0, 0, 0), (0, 2), "rejected"),               # d = 0
            ((0, 0, -0.5), (0, 0, 1e-30), (0, 2), "rejected"),           # len underflows to 0
            ((nan, 0, -0.5), (0, 0, 1), (0, 2), "rejected"), ((0, inf, -0.5), (0, 0, 1), (0, 2), "rejected"),
            ((0, 0, -0.5), (0, nan, 1), (0, 2), "rejected"), ((0, 0, -0.5), (0, 0, -inf), (0, 2), "rejected"),
            ((0, 0, -0.5), (0, 0, 1), (nan, 2), "rejected"), ((0, 0, -0.5), (0, 0, 1), (0, nan), "rejected"),
            ((0, 0, -0.5), (0, 0, 1), (-inf, 2), "rejected"), ((0, 0, -0.5), (0, 0, 1), (0, inf), "rejected"),
            ((0, 0, -0.5), (0, 0, 1), (2, 1), "rejected"),               # t0 > t1
            ((0, 0, -0.5), (0, 0, 1), (0.45, 0.45), STARTS_INSIDE),      # t0 == t1 inside the sphere
            ((0, 0, -0.5), (0, 0, 1), (0.39, 0.39), MISS),               # t0 == t1 in the box, outside the sphere: one evaluation
            ((0, 0, -0.5), (0, 0, 1), (0.1, 0.1), "rejected"),           # t0 == t1 in front of the box: an empty clip
            ((0.12, 0.12, -0.5), (0, 0, 1), (0, 2), MISS),               # along a box edge (x01 == 1 on two axes: in the slab)
            ((-0.5, 0.74, 0), (1, -1, 0), (0, 2), MISS),                 # touches the box edge x = y = hi in one point, or not at all
            ((0.3, 0, -0.5), (0, 0, 1), (0, 2), "rejected"),             # a box miss, the parallel axes outside
            ((0, 0, -0.5), (0.3, 0.3, -1), (0, 2), "rejected"),          # a box miss, pointing away
            ((0.01, 0.02, 0), (1, 0, 0), (0, 2), STARTS_INSIDE),         # starts inside the sphere
            ((0.1, 0, -0.5), (0, 0, 1), (0, 2), MISS)]                   # through the box beside the sphere
    o, d, tr = (np.array([r[i] for r in rows], np.float32) for i in range(3))
    return o, d, tr, [r[3] for r in rows]


def check_degenerate(t_hit, status, n_eval, sdf_hit, max_steps=128, n_bisect=8):
    o, d, tr, want = degenerate_rays()
    for r, w in enumerate(want):
        got = (int(status[r]), int(n_eval[r]), float(t_hit[r]), float(sdf_hit[r]))
        if w == "rejected":
            same_t = got[2] == float(tr[r, 0]) or (np.isnan(got[2]) and np.isnan(tr[r, 0]))
            assert got[0] == MISS and got[1] == 0 and same_t and got[3] == 0.0, (r, got)
        elif w == "hit":
            assert got[0] in (CONVERGED, BRACKETED) and (got[0] == BRACKETED or abs(got[3]) <= EPS), (r, got)
        else:
            assert got[0] == w, (r, got)
        if w != "rejected":
            assert 1 <= got[1] <= max_steps + n_bisect and tr[r, 0] <= got[2] <= tr[r, 1], (r, got)
