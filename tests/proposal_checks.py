"""Shared by tests/test_proposal_host.py (CPU twin against the rules restated with numpy) and tests/test_gpu_zzzzzzzzzzzzzzzproposal.py (kernels
against the twin): the host harness of the proposal loss between two packed lists (tests/host_harness/proposal/proposal_host.cpp over
lab4d_amd/csrc/proposal_math.hpp), the generator of the test lists, the rules of include/lab4d_proposal.h restated with numpy in float32,
and the float64 brute force -- the overlap sum over all pairs, the loss and the adjoint by the formula.  A helper module: no test in it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
from presample_checks import dir_length, prefix_f32, words  # noqa: E402,F401

TWIN = "proposal/proposal"  # tests/host_harness/proposal/proposal_host.cpp: a folder of its own (tests/test_host_twin.py pins the census of the twins beside it)
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 200)
RAYS = (1, 63, 64, 65, 1025)
EPS = float(np.finfo(np.float32).eps)
SENTINEL_F, SENTINEL_I = np.float32(-7.5), np.int32(-7)
BAR = 1e-4  # the project's fp32 parity bar: max |x - ref| / max |ref| per array
f32 = np.float32
# directions whose length is exact in fp32 (the squares and their sums are dyadic): 0.5, 1, 2 along an axis and 0.625, 1.25, 2.5 in a plane
_EXACT = [(0.5, 0, 0), (0, 1.0, 0), (0, 0, 2.0), (0.375, 0.5, 0), (0, 0.75, 1.0), (2.0, 0, 1.5)]


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def _layout(lengths, rng, gaps):
    gap = (rng.integers(0, 3, len(lengths)) == 0) * rng.integers(1, 4, len(lengths)) if gaps else np.zeros(len(lengths), np.int64)
    start = (np.cumsum(lengths + gap) - lengths).astype(np.int32)
    return start, lengths.astype(np.int32), int((lengths + gap).sum())


def make_case(R, seed, gaps=True):
    """Two packed lists of the same R rays, an envelope list `e` and a fine list `f`, each a dict of t, deltas, width (in t), w, start, count,
    P; and dir (R, 3).  Lengths: ray r < 64 has (n_e, n_f) = (LENGTHS[r % 8], LENGTHS[r // 8]) -- every pairing, the empty envelope with a
    fine list and the reverse included -- then both are drawn from LENGTHS; gaps of 1..3 unowned rows in front of a third of the rays, in
    each list on its own.  From the end: the last ray owns (P - 5, 65) in both lists, which leaves [0, P) and is cut to 5 rows (R = 1: that
    ray alone); with R >= 3 the ray before it starts at -3 in both lists (no rows) and the one before that has 65 and 65 rows and
    |dir| = 0.  Envelope rows sit on the lattice t = (k + 0.5) / 64 with k strictly ascending in steps of 1 or 2 (a step of 2 leaves a hole)
    and are 1 / 64 wide in t: they tile the lattice cells, exact in fp32.  Fine rows sit at t = m / 512, sorted, across the envelope's range
    and a little beyond, and are 0, 1 / 512, 1 / 256 or 1 / 128 wide: lo is not monotone, and intervals touch envelope edges exactly.
    deltas = width * |dir| rounded once.  Half of the rays have a direction whose length is exact in fp32 (0.5 .. 2.5: there the intervals are
    exact and the touches are real), the others a random direction of length near 0.5, 1 or 2.  Weights: uniform in [0, 1) with three in
    ten set to zero; in every ray of 63 rows or more one is NaN and one is negative, in each list.  numpy float32 / int32."""
    rng = np.random.default_rng(seed)
    n_special = min(R, 1) + (2 if R >= 3 else 0)
    n_plain = R - n_special
    ne = np.array([LENGTHS[r % 8] if r < 64 else rng.choice(LENGTHS) for r in range(n_plain)], np.int64).reshape(n_plain)
    nf = np.array([LENGTHS[r // 8] if r < 64 else rng.choice(LENGTHS) for r in range(n_plain)], np.int64).reshape(n_plain)
    if R >= 3:
        ne, nf = np.append(ne, [65, 0]), np.append(nf, [65, 0])
    d = rng.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([0.5, 1.0, 2.0], (R, 1))).astype(f32)
    exact = rng.random(R) < 0.5
    d[exact] = f32(_EXACT)[rng.integers(0, len(_EXACT), int(exact.sum()))] * rng.choice(f32([1, -1]), (int(exact.sum()), 1))
    if R >= 3:
        d[R - 3] = 0.0
    case = {"R": R, "dir": d}
    length = dir_length(d)
    for key, lengths in (("e", ne), ("f", nf)):
        start, count, P = _layout(lengths, rng, gaps)
        if R >= 3:
            start[-1], count[-1] = -3, 10
        if R >= 1:
            P += 5
            start, count = np.append(start, np.int32(P - 5)), np.append(count, np.int32(65))
        assert start.shape[0] == R
        lst = {"P": P, "start": start.astype(np.int32), "count": count.astype(np.int32), "t": rng.random(P).astype(f32), "width": np.full(P, 1.0 / 64.0, f32),
               "w": rng.random(P).astype(f32)}  # (the rows of no ray: anything)
        lst["w"][rng.random(P) < 0.3] = 0.0
        lst["deltas"] = lst["width"].copy()
        case[key] = lst
    for r in range(R):
        s, n = rows_of(case["e"], r)
        k = np.cumsum(rng.integers(1, 3, n))
        case["e"]["t"][s:s + n] = (k + 0.5) / 64.0
        top = int(k[-1]) + 2 if n else 8
        sf, nfr = rows_of(case["f"], r)
        case["f"]["t"][sf:sf + nfr] = np.sort(rng.integers(4, top * 8 + 1, nfr)) / 512.0
        case["f"]["width"][sf:sf + nfr] = rng.choice(f32([0.0, 1.0 / 512.0, 1.0 / 256.0, 1.0 / 128.0]), nfr)
        for lst in (case["e"], case["f"]):
            s, n = rows_of(lst, r)
            lst["deltas"][s:s + n] = lst["width"][s:s + n] * length[r]
            if n >= 63:
                lst["w"][s + 7], lst["w"][s + 40] = np.nan, -0.25
    return case


def rows_of(lst, r):
    s, n, P = int(lst["start"][r]), int(lst["count"][r]), lst["P"]
    if s < 0 or s >= P or n <= 0:
        return 0, 0
    return s, min(n, P - s)


def owned(lst, R):
    m = np.zeros(lst["P"], bool)
    for r in range(R):
        s, n = rows_of(lst, r)
        m[s:s + n] = True
    return m


def g_loss_of(R, seed=1):
    """an upstream gradient per ray: positive and negative values, a zero"""
    g = (np.random.default_rng(seed).standard_normal(R) * 2).astype(f32)
    g[R // 2] = 0.0
    return g


# ---------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data


def host_envelope(lib, case):
    e, R = case["e"], case["R"]
    out = {k: np.full(e["P"], SENTINEL_F, f32) for k in ("lo_e", "hi_e", "cdf_e")}
    lib.proposal_host_envelope(_p(e["w"]), _p(e["t"]), _p(e["deltas"]), _p(e["start"]), _p(e["count"]), _p(case["dir"]), R, e["P"], _p(out["lo_e"]), _p(out["hi_e"]),
                               _p(out["cdf_e"]))
    return out


def host_loss(lib, case, eps=EPS, g_loss=None):
    """the twin's three calls -> dict lo_e, hi_e, cdf_e, span, coef, loss, g_w_e; the sentinels stay in the rows of no ray"""
    e, f, R = case["e"], case["f"], case["R"]
    out = host_envelope(lib, case)
    out.update(span=np.full((f["P"], 2), SENTINEL_I, np.int32), coef=np.full(f["P"], SENTINEL_F, f32), loss=np.full(R, SENTINEL_F, f32),
               g_w_e=np.full(e["P"], SENTINEL_F, f32))
    lib.proposal_host_forward(_p(out["lo_e"]), _p(out["hi_e"]), _p(out["cdf_e"]), _p(e["start"]), _p(e["count"]), e["P"], _p(f["w"]), _p(f["t"]), _p(f["deltas"]),
                              _p(f["start"]), _p(f["count"]), f["P"], _p(case["dir"]), R, eps, _p(out["span"]), _p(out["coef"]), _p(out["loss"]))
    g = g_loss_of(R) if g_loss is None else g_loss
    lib.proposal_host_backward(_p(g), _p(out["span"]), _p(out["coef"]), _p(e["w"]), _p(e["start"]), _p(e["count"]), e["P"], _p(f["start"]), _p(f["count"]), f["P"], R,
                               _p(out["g_w_e"]))
    return out


def host_weights_backward(lib, density, deltas, start, count, P, g_w, g_trans=None):
    g = np.full(P, SENTINEL_F, f32)
    lib.proposal_host_weights_backward(_p(density), _p(deltas), _p(start), _p(count), start.shape[0], P, _p(g_w), _p(g_trans), _p(g))
    return g


# ---------------------------------------------------------------------------------------------------
# the rules with numpy, in float32
# ---------------------------------------------------------------------------------------------------
def count_before(v, x, or_equal):
    """the binary search of pmerge_math.hpp's count_before over the ascending values v, for every x at once"""
    lo, hi = np.zeros(x.shape[0], np.int64), np.full(x.shape[0], v.shape[0], np.int64)
    while (lo < hi).any():
        mid = lo + ((hi - lo) >> 1)
        m = v[np.minimum(mid, max(v.shape[0] - 1, 0))] if v.shape[0] else np.zeros(x.shape[0], f32)
        with np.errstate(invalid="ignore"):
            go = (lo < hi) & ((m <= x) if or_equal else (m < x))
        stay = (lo < hi) & ~go
        lo, hi = np.where(go, mid + 1, lo), np.where(stay, mid, hi)
    return lo


def intervals(lst, r, length):
    """INTERVAL for the rows of ray r -> lo, hi (float32)"""
    s, n = rows_of(lst, r)
    t, dl = lst["t"][s:s + n], lst["deltas"][s:s + n]
    h = f32(0.5) * (dl / length if length > 0 else np.zeros(n, f32))
    return (t - h).astype(f32), (t + h).astype(f32)


def positive(w):
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, w, f32(0)).astype(f32)


def ref_loss(case, eps=EPS, g_loss=None):
    """Every rule of include/lab4d_proposal.h but the weights adjoint -> host_loss's dict"""
    e, f, R = case["e"], case["f"], case["R"]
    out = {"lo_e": np.full(e["P"], SENTINEL_F, f32), "hi_e": np.full(e["P"], SENTINEL_F, f32), "cdf_e": np.full(e["P"], SENTINEL_F, f32),
           "span": np.full((f["P"], 2), SENTINEL_I, np.int32), "coef": np.full(f["P"], SENTINEL_F, f32), "loss": np.zeros(R, f32),
           "g_w_e": np.full(e["P"], SENTINEL_F, f32)}
    g = g_loss_of(R) if g_loss is None else g_loss
    length = dir_length(case["dir"]) if R else np.zeros(0, f32)
    eps = f32(eps)
    for r in range(R):
        se, n_e = rows_of(e, r)
        sf, n_f = rows_of(f, r)
        lo_e, hi_e = intervals(e, r, length[r])
        C = prefix_f32(positive(e["w"][se:se + n_e]))[0] if n_e else np.zeros(0, f32)
        out["lo_e"][se:se + n_e], out["hi_e"][se:se + n_e], out["cdf_e"][se:se + n_e] = lo_e, hi_e, C
        acc = np.zeros(n_e, f32)
        if n_f:
            lo, hi = intervals(f, r, length[r])
            j0, j1 = count_before(hi_e, lo, True), count_before(lo_e, hi, False)
            full = j1 > j0
            with np.errstate(invalid="ignore", over="ignore"):
                B = np.where(full, (C[np.maximum(j1 - 1, 0)] if n_e else f32(0)) - np.where(j0 > 0, C[np.maximum(j0 - 1, 0)] if n_e else f32(0), f32(0)), f32(0)).astype(f32)
                B = np.where(B < 0, f32(0), B).astype(f32)  # (a NaN stays)
                v = positive(f["w"][sf:sf + n_f])
                x = positive(v - B)
                den = np.where(x > 0, v + eps, f32(1)).astype(f32)
                l = np.where(x > 0, (x * x) / den, f32(0)).astype(f32)
                c = np.where(x > 0, (f32(-2) * x) / den, f32(0)).astype(f32)
            out["span"][sf:sf + n_f, 0], out["span"][sf:sf + n_f, 1], out["coef"][sf:sf + n_f] = j0, j1, c
            out["loss"][r] = prefix_f32(l)[1]
            for i in range(n_f):
                if full[i]:
                    acc[j0[i]:j1[i]] = acc[j0[i]:j1[i]] + g[r] * c[i]
        with np.errstate(invalid="ignore"):
            out["g_w_e"][se:se + n_e] = np.where(e["w"][se:se + n_e] > 0, acc, f32(0))
    return out


def assert_same(got, ref, what, keys=("lo_e", "hi_e", "cdf_e", "span", "coef", "loss", "g_w_e")):
    """the arrays by their words, the rows of no ray (sentinels) included"""
    for k in keys:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        a, b = (got[k], ref[k]) if k == "span" else (words(got[k]), words(ref[k]))
        assert np.array_equal(a, b), (what, k, int((a != b).sum()), np.flatnonzero((a != b).reshape(-1))[:5])


# ---------------------------------------------------------------------------------------------------
# the float64 brute force
# ---------------------------------------------------------------------------------------------------
def brute64(case, got, eps=EPS, g_loss=None):
    """The loss in float64 without a search and without a prefix.  The interval ends are data: the fp32 values the INTERVAL rule defines
    (got["lo_e"], got["hi_e"], and intervals() for the fine rows), taken as they are -- an end moved by a rounding would move a touching
    pair in or out of the overlap set and change the bound by a whole weight.  Everything behind them is float64: envelope row j overlaps
    fine row i iff lo_e_j < hi_i and lo_i < hi_e_j, tested for ALL pairs (a positive common length; a fine row of zero width counts where
    it lies strictly inside); B = the sum of max(w_e, 0) over the overlap set; the loss and the adjoint by the formula.
    -> dict overlap (list of (n_f, n_e) bool per ray), loss (R,), g_w_e (Pe,; 0 in the rows of no ray)"""
    e, f, R = case["e"], case["f"], case["R"]
    g = (g_loss_of(R) if g_loss is None else g_loss).astype(np.float64)
    length = dir_length(case["dir"]) if R else np.zeros(0, f32)
    out = {"overlap": [], "loss": np.zeros(R), "g_w_e": np.zeros(e["P"])}
    for r in range(R):
        se, n_e = rows_of(e, r)
        sf, n_f = rows_of(f, r)
        lo_e, hi_e = got["lo_e"][se:se + n_e].astype(np.float64), got["hi_e"][se:se + n_e].astype(np.float64)
        lo, hi = (a.astype(np.float64) for a in intervals(f, r, length[r]))
        O = (lo_e[None, :] < hi[:, None]) & (lo[:, None] < hi_e[None, :])
        out["overlap"].append(O)
        m, v = positive(e["w"][se:se + n_e]).astype(np.float64), positive(f["w"][sf:sf + n_f]).astype(np.float64)
        x = np.maximum(v - O @ m, 0.0)
        den = np.where(x > 0, v + np.float64(f32(eps)), 1.0)
        out["loss"][r] = (x * x / den).sum()
        out["g_w_e"][se:se + n_e] = np.where(m > 0, g[r] * ((-2.0 * x / den) @ O), 0.0)
    return out


def rel_err(x, ref):
    """the project's metric: max |x - ref| / max |ref| of one array"""
    return float(np.abs(np.asarray(x, np.float64) - ref).max(initial=0.0) / max(float(np.abs(ref).max(initial=0.0)), 1e-300))


# ---------------------------------------------------------------------------------------------------
# the weights adjoint in float64
# ---------------------------------------------------------------------------------------------------
def weights_case(R=65, seed=3):
    """a list of make_case's (its envelope) with a density in [0, 40) that holds a NaN, a negative and a zero value in ray 3, an upstream
    g_w (P,) and g_trans (R,)"""
    lst = make_case(R, seed)["e"]
    rng = np.random.default_rng(seed + 1)
    density = (rng.random(lst["P"]) * 40).astype(f32)
    s3, n3 = rows_of(lst, 3)
    assert n3 >= 63
    density[s3 + 1], density[s3 + 2], density[s3 + 5] = np.nan, -3.0, 0.0
    return lst, density, rng.standard_normal(lst["P"]).astype(f32), rng.standard_normal(R).astype(f32)


def weights_backward64(lst, density, g_w, g_trans=None):
    """float64 autograd through the oracle's compute_weights, ray by ray at the ray's own length -> g_density (P,), 0 in the rows of no ray
    and in the rows whose tau does not count (NaN or not > 0: the TAU rule gives them tau = 0, a constant)"""
    import torch
    from oracle import lab4d_oracle as O
    R = lst["start"].shape[0]
    out = np.zeros(lst["P"])
    for r in range(R):
        s, n = rows_of(lst, r)
        if n == 0:
            continue
        with np.errstate(invalid="ignore"):
            counted = (density[s:s + n] * lst["deltas"][s:s + n]) > 0
        d = torch.tensor(np.where(counted, density[s:s + n], 0.0).astype(np.float64), requires_grad=True)
        dl = torch.tensor(lst["deltas"][s:s + n].astype(np.float64))
        w, T = O.compute_weights(torch.where(torch.tensor(counted), d, torch.zeros_like(d))[None, :, None], dl[None, :, None])
        L = (w[0] * torch.tensor(g_w[s:s + n].astype(np.float64))).sum()
        if g_trans is not None:
            L = L + T[0, -1] * float(g_trans[r])
        L.backward()
        out[s:s + n] = d.grad.numpy()
    return out
