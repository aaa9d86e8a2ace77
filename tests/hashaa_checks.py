"""Shared by tests/test_hashaa_host.py (CPU twin against float64) and tests/test_gpu_zzzzzzzzzzzzzzzzzzhashaa.py (kernels against float64, with
the twin as the yardstick): the footprint-weighted hash encoding (include/lab4d_hashgrid.h, lab4d_amd/csrc/hashgrid_math.hpp level_weight).
Here: the inputs, the harness of the twin (tests/host_harness/hashaa/hashaa_host.cpp), a float64 reference in numpy that follows the definition to
the letter, the error measures, and a torch-CPU restatement of the weighted field.  A helper module: no test.

The float64 reference forms x * res in FLOAT32, as cell_of demands (the product is rounded before the cell is taken), and continues in float64
from that rounded product: reference and kernel then agree on every sample's cell, and NO sample is left out of any comparison.  The weights
are math.erf of the float64 quotient; the table and point gradients are accumulated in float64."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402

CONFIGS = {"a": (16, 2, 14, 16, 512), "b": (8, 4, 10, 4, 128)}  # (L, F, log2_T, n_min, n_max)
SIZES = (1, 63, 64, 65, 257, 1000)  # the wave and block edges of the wave-uniform backward
N_ROWS = 1000  # every size is a prefix of one set of rows: a sample's out and g_x do not depend on the rows around it
BIG = 65536  # the level-major dispatch of the inside-only forward starts here
PATTERNS = ("zero", "inf", "loguniform", "raylike", "alternating")
MIXED = PATTERNS[2:]
W_MINS = (0.0, 1.0 / 256.0)
SQRT8_F32 = float(np.float32(2.8284271))  # the constant of level_weight as the compilers read it
TABLE_FLOOR = 1e-6  # relative L2 of "equal up to the order of the atomics" (tests/test_gpu_zzhashgrid.py, the packed-fp16 test's dense levels)
FACTOR = 4.0  # device error <= 4 x the twin's: a 2-ulp erff and the order of the atomics


TWIN = "hashaa/hashaa"  # tests/host_harness/hashaa/hashaa_host.cpp: a folder of its own, as the other newer twins


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def res_list(name):
    L, _, _, n_min, n_max = CONFIGS[name]
    b = math.exp((math.log(n_max) - math.log(n_min)) / (L - 1)) if L > 1 else 1.0
    return [int(math.floor(n_min * b ** l + 1e-9)) for l in range(L)]


def table(name, seed=1):
    L, F, log2_T, _, _ = CONFIGS[name]
    return (np.random.default_rng(seed).standard_normal((L, 1 << log2_T, F)) * 0.1).astype(np.float32)


def points(n, seed=2):
    """(n,3) float32 in [0,1)^3; in front: x exactly 0, exactly 1, three rows outside the cube and a NaN row (an inside-only launch zeroes the
    last four, any other launch clamps them -- NaN to 0, as fmaxf does)"""
    x = np.random.default_rng(seed).random((n, 3)).astype(np.float32)
    special = np.array([[0, 0, 0], [1, 1, 1], [-0.3, 1.7, 0.5], [1.5, 0.5, 0.5], [0.5, -0.25, 0.5], [np.nan, 0.5, 0.5]], np.float32)
    k = min(n, len(special))
    x[:k] = special[:k]
    return x


def radius(pattern, n, seed=3):
    """(n,) float32.  zero / inf: every row.  loguniform: log-uniform in [1e-5, 10] per sample (mixed weights inside every wave), with a negative,
    a NaN and an infinite radius in rows 6..8.  raylike: constant up to a factor 2 and sorted inside every run of 64 rows, the runs at radii from
    0.002 to 50 -- whole waves are zero at the fine levels and non-zero at the coarse ones (w_min = 1/256 cuts where radius * res > 102), the
    skip path; run 0 is such a wave.  alternating: 0 in the even rows, log-uniform in [0.05, 5] in the odd ones."""
    rng = np.random.default_rng(seed)
    if pattern == "zero":
        return np.zeros(n, np.float32)
    if pattern == "inf":
        return np.full(n, np.inf, np.float32)
    if pattern == "loguniform":
        r = np.exp(rng.uniform(math.log(1e-5), math.log(10.0), n)).astype(np.float32)
        for i, v in ((6, -1.0), (7, np.nan), (8, np.inf)):
            if i < n:
                r[i] = v
        return r
    if pattern == "raylike":
        bases = np.array([1.0, 0.02, 5.0, 0.3, 0.002, 50.0])  # (run 0, radius 1 .. 2: cut from res 102 / 51 on, alive at res 4 and 16)
        run = np.arange(n) // 64
        within = np.sort(rng.uniform(1.0, 2.0, (run.max() + 1, 64)), axis=1).reshape(-1)[:n] if n else np.zeros(0)
        return (bases[run % len(bases)] * within).astype(np.float32)
    if pattern == "alternating":
        r = np.exp(rng.uniform(math.log(0.05), math.log(5.0), n)).astype(np.float32)
        r[0::2] = 0.0
        return r
    raise KeyError(pattern)


def cotangent(n, C, seed=4):
    return np.random.default_rng(seed).standard_normal((n, C)).astype(np.float32)


def inside01(x):
    with np.errstate(invalid="ignore"):
        return ((x >= 0) & (x <= 1)).all(-1)


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
def _c(a, dt=np.float32):
    return np.ascontiguousarray(a, dt)


def host_forward(lib, x, rad, tab, res, log2_T, w_min, inside_only):
    x, rad, tab, res = _c(x), _c(rad), _c(tab), _c(res, np.int32)
    S, (L, _, F) = x.shape[0], tab.shape
    out = np.full((S, L * F), np.nan, np.float32)
    assert lib.hashaa_host_forward(x.ctypes.data, rad.ctypes.data, tab.ctypes.data, res.ctypes.data, S, L, log2_T, F, w_min, int(inside_only), out.ctypes.data) == 0
    return out


def host_backward(lib, x, rad, tab, res, log2_T, w_min, g_out):
    x, rad, tab, res, g_out = _c(x), _c(rad), _c(tab), _c(res, np.int32), _c(g_out)
    S, (L, _, F) = x.shape[0], tab.shape
    g_table, g_x = np.zeros_like(tab), np.full((S, 3), np.nan, np.float32)
    assert lib.hashaa_host_backward(x.ctypes.data, rad.ctypes.data, tab.ctypes.data, res.ctypes.data, g_out.ctypes.data, S, L, log2_T, F, w_min,
                                    g_table.ctypes.data, g_x.ctypes.data) == 0
    return g_table, g_x


# ---------------------------------------------------------------------------------------------------
# the definition in numpy float64
# ---------------------------------------------------------------------------------------------------
_ERF = np.vectorize(math.erf, otypes=[np.float64])


def ref_weights(rad, res, w_min):
    """(S, L) float64: 1 where not radius > 0; erf(1 / (sqrt(8) radius res)) otherwise; 0 where that lies below w_min"""
    rad = np.asarray(rad, np.float32).astype(np.float64)[:, None]
    n = np.asarray(res, np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        pos = np.broadcast_to(rad > 0, (rad.shape[0], n.shape[1]))
    w = np.ones(pos.shape, np.float64)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        z = 1.0 / (SQRT8_F32 * rad * n)
    if pos.any():
        w[pos] = _ERF(z[pos])
    w[pos & (w < float(np.float32(w_min)))] = 0.0
    return w


def _vertices(i0, r, log2_T):
    """(8, S) int64 vertex indices and (8, 3) corner offsets"""
    n, T = r + 1, 1 << log2_T
    corners = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)], np.int64)
    v = i0[None, :, :] + corners[:, None, :]  # (8, S, 3)
    if n ** 3 <= T:
        return v[..., 0] + n * (v[..., 1] + n * v[..., 2]), corners
    m = 0xFFFFFFFF
    return (v[..., 0] ^ ((v[..., 1] * 2654435761) & m) ^ ((v[..., 2] * 805459861) & m)) & (T - 1), corners


def reference(x, rad, tab, res, log2_T, w_min, inside_only, g_out=None):
    """out (S, L*F) float64; with g_out also g_table (L, T, F) and g_x (S, 3) float64.  The adjoint knows no inside_only, like the kernels' (a
    caller masks the cotangent rows of the points it zeroed)."""
    x = np.asarray(x, np.float32)
    S, (L, T, F) = x.shape[0], tab.shape
    tab64 = tab.astype(np.float64)
    w = ref_weights(rad, res, w_min)
    xc = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(1))).astype(np.float32)
    keep = inside01(x) if inside_only else np.ones(S, bool)
    out = np.zeros((S, L, F), np.float64)
    if g_out is not None:
        g = np.asarray(g_out, np.float32).astype(np.float64).reshape(S, L, F) * w[:, :, None]
        g_table, g_x = np.zeros((L, T, F), np.float64), np.zeros((S, 3), np.float64)
    for l, r in enumerate(res):
        p = (xc * np.float32(r)).astype(np.float32).astype(np.float64)  # the product rounded in float32, then exact
        f = np.minimum(np.floor(p), r - 1)
        fr = p - f
        v, corners = _vertices(f.astype(np.int64), r, log2_T)
        ax = np.where(corners[:, None, :] == 1, fr[None], 1.0 - fr[None])  # (8, S, 3)
        wt = ax.prod(-1)  # (8, S)
        enc = (wt[:, :, None] * tab64[l][v]).sum(0)  # (S, F)
        out[:, l] = np.where((keep & (w[:, l] != 0))[:, None], enc * w[:, l, None], 0.0)
        if g_out is not None:
            np.add.at(g_table[l], v.reshape(-1), (wt[:, :, None] * g[None, :, l, :]).reshape(-1, F))
            dot = (tab64[l][v] * g[None, :, l, :]).sum(-1)  # (8, S)
            sign = np.where(corners == 1, 1.0, -1.0)  # (8, 3)
            g_x[:, 0] += (sign[:, 0, None] * ax[..., 1] * ax[..., 2] * dot).sum(0) * r
            g_x[:, 1] += (ax[..., 0] * sign[:, 1, None] * ax[..., 2] * dot).sum(0) * r
            g_x[:, 2] += (ax[..., 0] * ax[..., 1] * sign[:, 2, None] * dot).sum(0) * r
    out = out.reshape(S, L * F)
    return out if g_out is None else (out, g_table, g_x)


# ---------------------------------------------------------------------------------------------------
# error measures and the 4x-twin rule
# ---------------------------------------------------------------------------------------------------
def max_abs(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max()) if a.size else 0.0


def level_rel_l2(a, ref):
    """(L,) relative L2 per level of a table gradient; a level whose reference is all zero: 0 where `a` is all zero too, inf otherwise"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    num = np.sqrt(((a - ref) ** 2).sum((1, 2)))
    den = np.sqrt((ref ** 2).sum((1, 2)))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))


def cotangent_for(x, C, inside_only, seed=4):
    """a cotangent whose rows are zero where an inside-only launch zeroed the encoding (what the field's mask does)"""
    g = cotangent(x.shape[0], C, seed)
    if inside_only:
        g[~inside01(x)] = 0.0
    return g


_CASES = {}


def case(name, pattern, w_min, inside_only, n=N_ROWS):
    """The inputs of one (configuration, radius pattern, w_min, inside_only) over n rows, the float64 reference and the twin on ALL n rows, and
    the twin's error in out and g_x: computed once per process and shared (never written to).  The per-sample quantities of a size S <= n are
    rows [:S] of these; a table gradient depends on S and is formed by table_gradients()."""
    key = (name, pattern, w_min, bool(inside_only), n)
    if key not in _CASES:
        L, F, log2_T, _, _ = CONFIGS[name]
        res, tab, x, rad = res_list(name), table(name), points(n), radius(pattern, n)
        g = cotangent_for(x, L * F, inside_only) if n <= N_ROWS else None
        lib = build_host()
        c = {"cfg": CONFIGS[name], "res": res, "table": tab, "x": x, "radius": rad, "g_out": g, "w_min": w_min, "inside_only": bool(inside_only)}
        c["twin_out"] = host_forward(lib, x, rad, tab, res, log2_T, w_min, inside_only)
        if g is None:
            c["ref_out"] = reference(x, rad, tab, res, log2_T, w_min, inside_only)
        else:
            c["ref_out"], _, c["ref_gx"] = reference(x, rad, tab, res, log2_T, w_min, inside_only, g)
            c["twin_gx"] = host_backward(lib, x, rad, tab, res, log2_T, w_min, g)[1]
            c["yard_gx"] = max_abs(c["twin_gx"], c["ref_gx"])
        c["yard_out"] = max_abs(c["twin_out"], c["ref_out"])
        _CASES[key] = c
    return _CASES[key]


def table_gradients(c, S):
    """(reference (L,T,F) float64, twin float32, the twin's relative L2 per level) of the first S rows of a case"""
    _, _, log2_T, _, _ = c["cfg"]
    _, ref, _ = reference(c["x"][:S], c["radius"][:S], c["table"], c["res"], log2_T, c["w_min"], c["inside_only"], c["g_out"][:S])
    twin, _ = host_backward(build_host(), c["x"][:S], c["radius"][:S], c["table"], c["res"], log2_T, c["w_min"], c["g_out"][:S])
    return ref, twin, level_rel_l2(twin, ref)


def table_bound(twin_err):
    """per level: 4 x the twin's relative L2, and TABLE_FLOOR where that is smaller"""
    return np.maximum(FACTOR * twin_err, TABLE_FLOOR)


# ---------------------------------------------------------------------------------------------------
# the weighted field in torch on the CPU
# ---------------------------------------------------------------------------------------------------
def torch_weights(rad01, res, w_min):
    """(S, L) float32: the rule once more, in torch's float32 ops on the CPU"""
    r = rad01.to(torch.float32)[:, None]
    n = torch.tensor(res, dtype=torch.float32)[None, :]
    w = torch.erf(1.0 / (torch.tensor(2.8284271, dtype=torch.float32) * r * n))
    w = torch.where(w < torch.tensor(w_min, dtype=torch.float32), torch.zeros_like(w), w)
    return torch.where(r > 0, w, torch.ones_like(w))


def field_reference(P, cfg, xyz, dirs, rad, w_min, get_density=True):
    """hashfield.forward(radius=rad, w_min=w_min) restated: the project's oracle encoding (oracle/hashgrid_oracle.py hash_encode) times the
    float32 weights of the metric radius over the box's smallest edge, then the Linears of HO.hash_field_forward"""
    import torch.nn.functional as F
    from oracle import hashgrid_oracle as HO
    lo, hi = P["aabb"][0], P["aabb"][1]
    x01 = (xyz - lo) / (hi - lo)
    res = HO.level_resolutions(cfg["L"], cfg["n_min"], cfg["n_max"])
    w = torch_weights(rad / (hi - lo).min(), res, w_min)
    enc = HO.hash_encode(x01, P["hash.table"], res, cfg["log2_T"]) * w.repeat_interleave(cfg["F"], -1)
    h = F.relu(F.linear(enc, P["hash.geo.0.weight"], P["hash.geo.0.bias"]))
    geo = F.linear(h, P["hash.geo.2.weight"], P["hash.geo.2.bias"])
    sdf = geo[:, :1]
    c = torch.cat([geo, dirs], -1)
    c = F.relu(F.linear(c, P["hash.color.0.weight"], P["hash.color.0.bias"]))
    c = F.relu(F.linear(c, P["hash.color.2.weight"], P["hash.color.2.bias"]))
    rgb = torch.sigmoid(F.linear(c, P["hash.color.4.weight"], P["hash.color.4.bias"]))
    inside = ((x01 >= 0) & (x01 <= 1)).all(-1, keepdim=True).to(rgb.dtype)
    if not get_density:
        return rgb * inside, sdf
    ibeta = P["logibeta"].exp()
    density = (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() * ibeta)) * ibeta
    return rgb * inside, density * inside
