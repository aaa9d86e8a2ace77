"""Shared by tests/test_hashsdf_host.py (CPU twin against float64) and tests/test_gpu_zzzzzzzhashsdf.py (kernels against float64): the host
harness of the hash field's SDF gradient (tests/host_harness/hashsdf_host.cpp over lab4d_amd/csrc/hashsdf_math.hpp), the test inputs, and
the truth: float64 torch autograd on the CPU over oracle/hashgrid_oracle.py -- hash_encode, the two Linears, autograd.grad(create_graph=True)
for the gradient in the point, a second autograd.grad for the parameter gradients.  Nothing of the code under test enters the truth."""
import functools

import numpy as np
import torch

import host_twin
from oracle import hashgrid_oracle as HO

TOL = 1e-4  # relative L2 per tensor: the project's fp32 bar (README.md)
CONFIGS = {"a": {"L": 16, "F": 2, "n_min": 4, "n_max": 128, "log2_T": 12},   # levels 0-5 dense, 6-15 hashed with heavy collisions
           "b": {"L": 16, "F": 2, "n_min": 16, "n_max": 512, "log2_T": 14}}
PARAMS = ("hash.table", "hash.geo.0.weight", "hash.geo.0.bias", "hash.geo.2.weight", "hash.geo.2.bias")
NEAR = 1e-4      # points with x01 * res_l within this of an integer are dropped: fp32 and float64 may pick different cells there
MAX_DROP = 0.02


def build_host():
    return host_twin.load("hashsdf")


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def res_list(cfg):
    return HO.level_resolutions(cfg["L"], cfg["n_min"], cfg["n_max"])


@functools.lru_cache(None)
def field(name, unit_box=True, zero_table=False):
    """P (float32, CPU), cfg: hashfield.make_weights with the table x 1e3, so that |grad sdf| is of order 1 and the eikonal gradient does
    not test the "- 1" alone.  unit_box: aabb = [0,1]^3, so that x01 == xyz and grad == grad01.  Shared: never modified."""
    from lab4d_amd import hashfield
    P, cfg = hashfield.make_weights(seed=3, cfg=CONFIGS[name])
    P["hash.table"] = torch.zeros_like(P["hash.table"]) if zero_table else P["hash.table"] * 1e3
    if unit_box:
        P["aabb"] = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    return P, cfg


def near_cell_face(P, cfg, xyz):
    """(S,) bool: x01 * res_l lies within NEAR of an integer on some axis at some level, with x01 formed in float32 (as the field does) or
    in float64 (as the truth does)"""
    lo, hi = P["aabb"][0], P["aabb"][1]
    bad = torch.zeros(xyz.shape[0], dtype=torch.bool)
    for x01 in (((xyz - lo) / (hi - lo)).double(), (xyz.double() - lo.double()) / (hi.double() - lo.double())):
        for r in res_list(cfg):
            p = x01 * r
            bad |= ((p - p.round()).abs() < NEAR).any(-1)
    return bad


def points(P, cfg, n, seed):
    """n points uniform in the box (float32, the field's frame), those near a cell face dropped; asserts the cap on the dropped share"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = P["aabb"][0], P["aabb"][1]
    cand = lo + torch.rand(n + max(16, n // 8), 3, generator=g) * (hi - lo)
    cand = torch.minimum(torch.maximum(cand, lo), hi)
    bad = near_cell_face(P, cfg, cand)
    share = float(bad.float().mean())
    assert share < MAX_DROP, share
    keep = cand[~bad]
    assert keep.shape[0] >= n
    return keep[:n].contiguous(), share


def ray_points(P, cfg, n=130):
    """n consecutive samples of one ray through the box (those near a cell face skipped)"""
    lo, hi = P["aabb"][0], P["aabb"][1]
    t = torch.linspace(0.02, 0.98, n + 12)[:, None]
    a, b = torch.tensor([0.03, 0.11, 0.07]), torch.tensor([0.96, 0.71, 0.88])
    pts = lo + (a + t * (b - a)) * (hi - lo)
    pts = pts[~near_cell_face(P, cfg, pts)]
    assert pts.shape[0] >= n
    return pts[:n].contiguous()


def cotangents(S, seed):
    g = torch.Generator().manual_seed(seed + 4242)
    return torch.randn(S, 1, generator=g), torch.randn(S, 3, generator=g)


def rel_l2(got, want):
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    d = float((got - want).norm())
    n = float(want.norm())
    return d / n if n > 0 else d


# ---------------------------------------------------------------------------------------------------
# the truth: float64 autograd over the oracle's encoding
# ---------------------------------------------------------------------------------------------------
def truth(P, cfg, xyz, g_sdf=None, g_grad=None, eikonal=False):
    """dict: sdf (S,1), grad (S,3) = d sdf / d xyz, and -- under the cotangents g_sdf (S,1) / g_grad (S,3), or for eikonal=True under
    ((|grad| - 1)^2 * inside).mean() -- the gradient of every parameter in PARAMS (zeros where the graph does not reach), `loss` (S,1)."""
    P64 = {k: v.double() for k, v in P.items()}
    leaves = [P64[k].clone().requires_grad_(True) for k in PARAMS]
    T, W1, b1, W2, B2 = leaves
    x = xyz.double().clone().requires_grad_(True)
    lo, hi = P64["aabb"][0], P64["aabb"][1]
    x01 = (x - lo) / (hi - lo)
    inside = ((x01 >= 0) & (x01 <= 1)).all(-1, keepdim=True).double()
    enc = HO.hash_encode(x01, T, res_list(cfg), cfg["log2_T"]) * inside
    h = torch.relu(torch.nn.functional.linear(enc, W1, b1))
    sdf = torch.nn.functional.linear(h, W2, B2)[:, :1]
    grad, = torch.autograd.grad(sdf.sum(), x, create_graph=True)
    out = {"sdf": sdf.detach(), "grad": grad.detach()}
    loss = None
    if eikonal:
        out["loss"] = ((grad.norm(2, -1, keepdim=True) - 1) ** 2 * inside).detach()
        loss = ((grad.norm(2, -1, keepdim=True) - 1) ** 2 * inside).mean()
    elif g_sdf is not None or g_grad is not None:
        loss = 0.0
        if g_sdf is not None:
            loss = loss + (sdf * g_sdf.double()).sum()
        if g_grad is not None:
            loss = loss + (grad * g_grad.double()).sum()
    if loss is not None:
        gs = torch.autograd.grad(loss, leaves, allow_unused=True)
        for k, leaf, g in zip(PARAMS, leaves, gs):
            out[k] = torch.zeros_like(leaf) if g is None else g.detach()
    return out


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), np.float32)


def _net(P):
    return (_np(P["hash.geo.0.weight"]), _np(P["hash.geo.0.bias"]), _np(P["hash.geo.2.weight"][0]), _np(P["hash.geo.2.bias"][:1]))


def host_forward(lib, P, cfg, x01):
    """the twin's sdf (S,1) and grad01 (S,3), torch float32"""
    x, table = _np(x01), _np(P["hash.table"])
    res = np.array(res_list(cfg), np.int32)
    W1, b1, w2, b2 = _net(P)
    S = x.shape[0]
    sdf, g = np.full(S, 7.0, np.float32), np.full((S, 3), 7.0, np.float32)
    rc = lib.hashsdf_host_forward(x.ctypes.data, table.ctypes.data, res.ctypes.data, S, cfg["L"], cfg["log2_T"], cfg["F"], W1.ctypes.data, b1.ctypes.data,
                                  w2.ctypes.data, b2.ctypes.data, sdf.ctypes.data, g.ctypes.data)
    assert rc == 0
    return torch.from_numpy(sdf)[:, None], torch.from_numpy(g)


def host_backward(lib, P, cfg, x01, g_sdf=None, g_grad01=None, n_rows=3, want=PARAMS):
    """the twin's parameter gradients under the cotangents, dict over `want`; the head's gradient is laid out like hash.geo.2.* (16 rows,
    row 0 from the twin, the others zero: the twin, like the kernels, sees row 0 only)"""
    x, table = _np(x01), _np(P["hash.table"])
    res = np.array(res_list(cfg), np.int32)
    W1, b1, w2, _ = _net(P)
    S = x.shape[0]
    gs = None if g_sdf is None else _np(g_sdf).reshape(-1)
    gg = None if g_grad01 is None else _np(g_grad01)
    out = {"hash.table": np.zeros_like(table), "hash.geo.0.weight": np.full_like(W1, 7.0), "hash.geo.0.bias": np.full_like(b1, 7.0),
           "w2": np.full_like(w2, 7.0), "b2": np.full(1, 7.0, np.float32)}
    names = {"hash.table": "hash.table", "hash.geo.0.weight": "hash.geo.0.weight", "hash.geo.0.bias": "hash.geo.0.bias", "hash.geo.2.weight": "w2",
             "hash.geo.2.bias": "b2"}
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    args = [out[names[k]] if k in want else None for k in PARAMS]
    rc = lib.hashsdf_host_backward(x.ctypes.data, table.ctypes.data, res.ctypes.data, S, cfg["L"], cfg["log2_T"], cfg["F"], W1.ctypes.data, b1.ctypes.data,
                                   w2.ctypes.data, ptr(gs), ptr(gg), *[ptr(a) for a in args], int(n_rows))
    assert rc == 0
    r = {}
    for k in want:
        a = torch.from_numpy(out[names[k]])
        if k == "hash.geo.2.weight":
            a = torch.cat([a[None], torch.zeros(15, 64)])
        if k == "hash.geo.2.bias":
            a = torch.cat([a, torch.zeros(15)])
        r[k] = a
    return r


def eikonal_cotangent(grad, inside):
    """d mean((|g| - 1)^2 * inside) / d g in float64 (zero where g == 0, torch's subgradient of the norm), as float32"""
    g = grad.double()
    n = g.norm(2, -1, keepdim=True)
    d = torch.where(n > 0, 2 * (n - 1) * g / n.clamp_min(1e-300), torch.zeros_like(g)) * inside.double() / g.shape[0]
    return d.float()
