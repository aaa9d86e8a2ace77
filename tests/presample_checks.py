"""Shared by tests/test_presample_host.py (CPU twin against the rules restated with numpy) and tests/test_gpu_zzzzzzzzzzzzzzpresample.py (kernels
against the twin): the host harness of the importance resampling of a packed list (tests/host_harness/presample/presample_host.cpp over
lab4d_amd/csrc/presample_math.hpp), the generator of the test lists, the rules of include/lab4d_presample.h restated with numpy in float32,
and the float64 piecewise-linear CDF that the emitted depths are judged in.  A helper module: no test in it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402

TWIN = "presample/presample"  # tests/host_harness/presample/presample_host.cpp: a folder of its own (tests/test_host_twin.py pins the census of the twins beside it)
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 200)
RAYS = (1, 63, 64, 65, 1025)
N_IMP = (1, 2, 64, 65, 130)
EPS = 1e-5
PAD = 5  # rows behind the capacity in every output buffer: they must keep their sentinel
SENTINEL_F, SENTINEL_I = np.float32(-7.5), np.int32(-7)
AABB = np.array([-0.12, -0.10, -0.15, 0.12, 0.14, 0.09], np.float32)
OUT_F, OUT_I = ("t", "deltas", "xyz", "dirs"), ("ray_idx", "src_row")
CDF_BAR = 1e-4  # the project's fp32 parity bar, absolute in the CDF domain [0, 1]
f32 = np.float32


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def dir_length(d):
    """|d| as ray_math.hpp forms it: the float32 root of the three rounded squares added x, then y, then z"""
    d = np.asarray(d, f32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def make_list(R, seed, gaps=True):
    """A packed list of R rays with weights.  Lengths: LENGTHS in turn for the first rays, then drawn from LENGTHS; gaps of 1..3 unowned rows
    in front of a third of the rays.  From the end: the last ray owns (P - 5, 65), which leaves [0, P) and is cut to 5 rows (R = 1: that ray
    alone); with R >= 3 the ray before it starts at -3 (no rows) and the one before that has 65 rows whose weights are all zero.  A ray's
    rows sit on the lattice t = k / 64 with k strictly ascending from 1 (steps of 1 or 2) and are 1 / 64 or 1 / 128 wide in t: disjoint
    intervals, exact in fp32 (`width`, in t; deltas = width * |dir| rounded once).  dir has a length near 0.5, 1 or 2.  Weights: uniform in
    [0, 1) with three in ten set to zero; in every ray of 63 rows or more one is NaN and one is negative.  numpy float32 / int32."""
    rng = np.random.default_rng(seed)
    n_special = min(R, 1) + (2 if R >= 3 else 0)
    n_plain = R - n_special
    lengths = np.array([LENGTHS[r % len(LENGTHS)] if r < 2 * len(LENGTHS) else rng.choice(LENGTHS) for r in range(n_plain)], np.int64).reshape(n_plain)
    if R >= 3:
        lengths = np.append(lengths, [65, 0])
    gap = (rng.integers(0, 3, len(lengths)) == 0) * rng.integers(1, 4, len(lengths)) if gaps else np.zeros(len(lengths), np.int64)
    start = (np.cumsum(lengths + gap) - lengths).astype(np.int32)
    count = lengths.astype(np.int32)
    P = int((lengths + gap).sum())
    if R >= 3:
        start[-1], count[-1] = -3, 10
    if R >= 1:
        P += 5
        start, count = np.append(start, np.int32(P - 5)), np.append(count, np.int32(65))
    assert start.shape[0] == R
    d = rng.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([0.5, 1.0, 2.0], (R, 1))).astype(f32)
    case = {"R": R, "P": P, "start": start.astype(np.int32), "count": count.astype(np.int32), "aabb": AABB,
            "origin": (rng.standard_normal((R, 3)) * 0.1).astype(f32), "dir": d,
            "t": rng.random(P).astype(f32), "width": np.full(P, 1.0 / 64.0, f32), "weights": rng.random(P).astype(f32)}  # (the rows of no ray: anything)
    case["weights"][rng.random(P) < 0.3] = 0.0
    case["deltas"] = case["width"].copy()
    length = dir_length(d)
    for r in range(R):
        s, n = rows_of(case, r)
        case["t"][s:s + n] = np.cumsum(rng.integers(1, 3, n)) / 64.0
        case["width"][s:s + n] = rng.choice(f32([1.0 / 64.0, 1.0 / 128.0]), n)
        case["deltas"][s:s + n] = case["width"][s:s + n] * length[r]
        if n >= 63:
            case["weights"][s + 7], case["weights"][s + 40] = np.nan, -0.25
        if R >= 3 and r == R - 3:
            case["weights"][s:s + n] = 0.0
    return case


def rows_of(case, r):
    s, n, P = int(case["start"][r]), int(case["count"][r]), case["P"]
    if s < 0 or s >= P or n <= 0:
        return 0, 0
    return s, min(n, P - s)


def uniforms(case, n_imp, seed):
    """a caller's u (R, n_imp): sorted per ray, a few below 0 and above 1 (clamped by the rule)"""
    rng = np.random.default_rng(seed)
    return np.sort(rng.random((case["R"], n_imp)) * 1.1 - 0.05, axis=1).astype(f32)


def unsorted_uniforms(case, n_imp, seed):
    """a caller's u (R, n_imp) that breaks the precondition: NOT sorted, one in ten outside [0, 1] on either side, a NaN in every ray (two
    with n_imp >= 66: one in each of the first two 64-sample chunks).  Only the ORDER rule's running maximum makes t non-decreasing here."""
    rng = np.random.default_rng(seed)
    u = (rng.random((case["R"], n_imp)) * 1.25 - 0.125).astype(f32)
    u[:, n_imp // 3] = np.nan
    if n_imp >= 66:
        u[:, 65] = np.nan
    return u


def _p(a):
    return None if a is None else a.ctypes.data


def host_weights(lib, density, deltas, start, count, P):
    """the twin's weights pass -> (w (P,) with the sentinel in the rows of no ray, trans (R,))"""
    R = start.shape[0]
    w, trans = np.full(P, SENTINEL_F, f32), np.full(R, SENTINEL_F, f32)
    lib.presample_host_weights(_p(density), _p(deltas), _p(start), _p(count), R, P, _p(w), _p(trans))
    return w, trans


def empty_buffers(case, cap, pad=PAD):
    out = {"t": np.full(cap + pad, SENTINEL_F, f32), "deltas": np.full(cap + pad, SENTINEL_F, f32), "xyz": np.full((cap + pad, 3), SENTINEL_F, f32),
           "dirs": np.full((cap + pad, 3), SENTINEL_F, f32), "ray_idx": np.full(cap + pad, SENTINEL_I, np.int32), "src_row": np.full(cap + pad, SENTINEL_I, np.int32),
           "ray_count": np.full(case["R"], SENTINEL_I, np.int32), "total": np.full(1, SENTINEL_I, np.int32), "overflow": np.full(1, 7, np.uint8)}
    return out


def host_count(lib, case, n_imp, eps=EPS):
    """the twin's count pass -> cdf (P,) with the sentinel in the rows of no ray, mass (R,), count (R,)"""
    cdf, mass, count = np.full(case["P"], SENTINEL_F, f32), np.full(case["R"], SENTINEL_F, f32), np.full(case["R"], SENTINEL_I, np.int32)
    lib.presample_host_count(_p(case["weights"]), _p(case["start"]), _p(case["count"]), case["R"], case["P"], n_imp, eps, _p(cdf), _p(mass), _p(count))
    return cdf, mass, count


def host_resample(lib, case, n_imp, u=None, eps=EPS, cap=None, pad=PAD):
    """The twin's two passes around numpy's exclusive sum.  cap None: the total.  -> dict with the fields of a lab4d_amd.packed.PrunedRays
    (numpy; the row buffers have cap + pad rows, the last `pad` of which the twin must leave alone; total an int, overflow a bool) and cdf,
    mass, count of the count pass."""
    R = case["R"]
    cdf, mass, count = host_count(lib, case, n_imp, eps)
    incl = np.cumsum(count, dtype=np.int64)
    start = (incl - count).astype(np.int32)
    if cap is None:
        cap = int(incl[-1]) if R else 0
    out = empty_buffers(case, cap, pad)
    o = lambda k: out[k].ctypes.data
    lib.presample_host_write(_p(case["weights"]), _p(cdf), _p(mass), _p(case["t"]), _p(case["deltas"]), _p(case["start"]), _p(case["count"]), _p(start), R, case["P"],
                             _p(case["origin"]), _p(case["dir"]), _p(u), n_imp, eps, cap, _p(case["aabb"]), o("t"), o("deltas"), o("xyz"), o("dirs"), o("ray_idx"),
                             o("src_row"), o("ray_count"), o("total"), o("overflow"))
    out.update(ray_start=start, total=int(out["total"][0]), overflow=bool(out["overflow"][0]), cdf=cdf, mass=mass, count=count, R=R, cap=cap)
    return out


# ---------------------------------------------------------------------------------------------------
# the rules with numpy, in float32
# ---------------------------------------------------------------------------------------------------
def prefix_f32(v):
    """the PREFIX order of include/lab4d_prune.h: chunks of 64, the doubling scan, then + carry -> (inclusive values, the last one)"""
    n, out, carry = v.shape[0], np.empty(v.shape[0], f32), f32(0)
    for j0 in range(0, n, 64):
        c = np.zeros(64, f32)
        c[:min(64, n - j0)] = v[j0:j0 + 64]
        for o in (1, 2, 4, 8, 16, 32):
            c[o:] = c[o:] + c[:-o]  # (the right side is formed from the values of the step before)
        c = c + carry
        out[j0:j0 + 64] = c[:n - j0]
        carry = c[63]
    return out, carry


def masses(case, eps=EPS):
    w = case["weights"]
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, w, f32(0)).astype(f32) + f32(eps)


def count_before_or_equal(C, q):
    """#{i : C_i <= q} by the binary search of pmerge_math.hpp's count_before, for every q at once"""
    lo, hi = np.zeros(q.shape[0], np.int64), np.full(q.shape[0], C.shape[0], np.int64)
    while (lo < hi).any():
        mid = lo + ((hi - lo) >> 1)
        with np.errstate(invalid="ignore"):
            go = (lo < hi) & (C[np.minimum(mid, C.shape[0] - 1)] <= q)
        stay = (lo < hi) & ~go
        lo, hi = np.where(go, mid + 1, lo), np.where(stay, mid, hi)
    return lo


def ref_resample(case, n_imp, u=None, eps=EPS):
    """Every rule of include/lab4d_presample.h at an unlimited capacity -> dict: cdf (the sentinel in the rows of no ray), mass, count,
    ray_start, total, and the rows t, deltas, xyz, dirs, ray_idx, src_row (total rows), u (the queries used, total), t_placed (t' of the PLACE rule, before ORDER's running maximum), monotone (R,) bool: the
    ray's prefixes never decrease."""
    R, P = case["R"], case["P"]
    m = masses(case, eps)
    cdf, mass, count = np.full(P, SENTINEL_F, f32), np.zeros(R, f32), np.zeros(R, np.int32)
    rows = {k: [] for k in OUT_F + OUT_I + ("u", "t_placed")}
    monotone = np.ones(R, bool)
    length = dir_length(case["dir"]) if R else np.zeros(0, f32)
    for r in range(R):
        s, n = rows_of(case, r)
        if n == 0:
            continue
        C, W = prefix_f32(m[s:s + n])
        cdf[s:s + n], mass[r] = C, W
        monotone[r] = bool((np.diff(C) >= 0).all())
        if not W > 0:
            continue
        count[r] = n_imp
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if u is None:
                uk = (np.arange(n_imp, dtype=f32) + f32(0.5)) / f32(n_imp)
            else:
                uk = np.where(u[r] > 0, np.where(u[r] < 1, u[r], f32(1)), f32(0)).astype(f32)
            q = uk * W
            i = np.minimum(count_before_or_equal(C, q), n - 1)
            E = np.where(i > 0, C[np.maximum(i - 1, 0)], f32(0))
            mi, di, ti = m[s + i], case["deltas"][s + i], case["t"][s + i]
            f = (q - E) / mi
            f = np.where(f > 0, np.where(f < 1, f, f32(1)), f32(0)).astype(f32)
            width = di / length[r] if length[r] > 0 else np.zeros(n_imp, f32)
            placed = ti + (f - f32(0.5)) * width
            tk = np.maximum.accumulate(placed)
            span = (di * W) / (f32(n_imp) * mi)
            span = np.where(span < di, span, di)
            d = case["dir"][r]
            unit = d / length[r] if length[r] > 0 else np.zeros(3, f32)
        rows["t"].append(tk), rows["deltas"].append(span), rows["u"].append(uk), rows["t_placed"].append(placed)
        rows["xyz"].append(case["origin"][r][None, :] + tk[:, None] * d[None, :]), rows["dirs"].append(np.broadcast_to(unit, (n_imp, 3)))
        rows["ray_idx"].append(np.full(n_imp, r, np.int32)), rows["src_row"].append((s + i).astype(np.int32))
    out = {k: (np.concatenate(v) if v else np.zeros((0, 3) if k in ("xyz", "dirs") else 0, np.int32 if k in OUT_I else f32)) for k, v in rows.items()}
    assert all(out[k].dtype == (np.int32 if k in OUT_I else f32) for k in out)
    incl = np.cumsum(count, dtype=np.int64)
    out.update(cdf=cdf, mass=mass, count=count, ray_start=(incl - count).astype(np.int32), total=int(incl[-1]) if R else 0, monotone=monotone, R=R)
    return out


def under_cap(case, full, cap, pad=PAD):
    """what the write call leaves in sentinel-filled buffers of cap + pad rows, given ref_resample's rows: the same dict as host_resample"""
    out = empty_buffers(case, cap, pad)
    total = full["total"]
    m = min(total, cap)
    for k in OUT_F + OUT_I:
        out[k][:m] = full[k][:m]
    park = np.array([AABB[3 + a] + (AABB[3 + a] - AABB[a]) for a in range(3)], f32)
    out["t"][m:cap], out["deltas"][m:cap], out["xyz"][m:cap], out["dirs"][m:cap], out["ray_idx"][m:cap], out["src_row"][m:cap] = 0, 0, park, f32([0, 0, 1]), -1, -1
    out["ray_count"][:] = np.clip(cap - full["ray_start"].astype(np.int64), 0, full["count"])
    out.update(ray_start=full["ray_start"], total=total, overflow=total > cap, cdf=full["cdf"], mass=full["mass"], count=full["count"], R=case["R"], cap=cap)
    return out


def capacities(full):
    """total, total - 1, a cut in the middle of a ray (the middle one of the rays with rows), 0"""
    total, live = full["total"], np.flatnonzero(full["count"])
    mid = int(full["ray_start"][live[len(live) // 2]]) + int(full["count"][live[len(live) // 2]]) // 2 if len(live) else 0
    return sorted({total, max(total - 1, 0), mid, 0})


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, ref, what):
    """every output of both calls, the floats by their words, the rows behind the capacity and the rows of no ray included"""
    assert got["total"] == ref["total"] and got["overflow"] == ref["overflow"] and got["cap"] == ref["cap"], (what, got["total"], ref["total"])
    for k in ("count", "ray_start", "ray_count") + OUT_I:
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k)
    for k in ("cdf", "mass") + OUT_F:
        assert got[k].dtype == f32 and got[k].shape == ref[k].shape and np.array_equal(words(got[k]), words(ref[k])), (what, k, int((words(got[k]) != words(ref[k])).sum()))


# ---------------------------------------------------------------------------------------------------
# the CDF domain, in float64
# ---------------------------------------------------------------------------------------------------
def cdf64(t_lo, t_hi, m, x):
    """F(x) of the piecewise-linear CDF whose row i carries the mass m_i spread evenly over [t_lo_i, t_hi_i] (ascending, disjoint), float64"""
    t_lo, t_hi, m, x = (np.asarray(a, np.float64) for a in (t_lo, t_hi, m, x))
    frac = np.clip((x[:, None] - t_lo[None, :]) / (t_hi - t_lo)[None, :], 0.0, 1.0)
    return (frac * m[None, :]).sum(1) / m.sum()


def cdf_errors(case, got, eps=EPS):
    """max over the emitted rows of |F64(t_k) - u_k|, per ray -> (R,) (0 for a ray that emitted nothing); got: ref_resample's dict or
    host_resample's at an unlimited capacity together with `u`"""
    m = masses(case, eps).astype(np.float64)
    err = np.zeros(case["R"])
    for r in range(case["R"]):
        s, n = rows_of(case, r)
        a, c = int(got["ray_start"][r]), int(got["count"][r])
        if c == 0:
            continue
        t, w = case["t"][s:s + n].astype(np.float64), case["width"][s:s + n].astype(np.float64)
        err[r] = np.abs(cdf64(t - w / 2, t + w / 2, m[s:s + n], got["t"][a:a + c]) - got["u"][a:a + c]).max()
    return err
