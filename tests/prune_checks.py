"""Shared by tests/test_prune_host.py (CPU twin against float64) and tests/test_gpu_zzzzzzzzprune.py (kernels against the twin): the host
harness of the prune (tests/host_harness/prune/prune_host.cpp over lab4d_amd/csrc/prune_math.hpp), the generator of the test lists, and the rules
of include/lab4d_prune.h restated in float64 numpy.  A helper module: no test in it."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402

AABB = np.array([-0.12, -0.10, -0.15, 0.12, 0.14, 0.09], np.float32)
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 200)
EPS = (1e-4, 1e-2)
ALPHA = (0.0, 1e-3, 0.05)
# A ray is generic when no float64 exclusive prefix lies within MARGIN (relative) of tau_stop and no tau within MARGIN of tau_min.  At 200
# rows an fp32 prefix passes through at most 6 scan adds, 4 carry adds and one product: under 12 roundings of 2^-24, about 7e-7 relative;
# the margin is roughly 14 times that.
MARGIN = 1e-5


TWIN = "prune/prune"  # tests/host_harness/prune/prune_host.cpp: a folder of its own (tests/test_host_twin.py pins the census of the twins beside it)


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def f32(x):
    return float(np.float32(x))


def thresholds(eps, alpha):
    """(tau_stop, tau_min) as lab4d_amd.packed.prune_thresholds forms them: double precision, rounded to fp32 once"""
    return (f32(-math.log(eps)) if eps > 0 else math.inf), f32(-math.log1p(-alpha))


def make_list(R, seed, gaps=True, out_of_range=True, density_max=200.0):
    """A packed list of R rays: lengths drawn from LENGTHS (R >= 8: each at least once), gaps of 1..3 unowned rows in front of a third of
    the rays, and (out_of_range) five rows behind the last ray that a (start, count) with count 65 owns -- it leaves [0, P) and is cut to 5
    -- or, for R = 1, that ray alone; and with R >= 3 one ray whose start lies in front of the list.  deltas 1/64, densities uniform in
    [0, density_max] (times a per-ray factor, below): tau averages 1.56 on seven rays in ten, which reach tau_stop = 9.2 after about six
    rows.  numpy float32 / int32."""
    rng = np.random.default_rng(seed)
    n_plain = max(R - (1 if out_of_range else 0) - (1 if out_of_range and R >= 3 else 0), 0)
    lengths = rng.choice(LENGTHS, n_plain)
    if n_plain >= len(LENGTHS):
        lengths[rng.permutation(n_plain)[:len(LENGTHS)]] = LENGTHS
    gap = (rng.integers(0, 3, n_plain) == 0) * rng.integers(1, 4, n_plain) if gaps else np.zeros(n_plain, np.int64)
    start = (np.cumsum(lengths + gap) - lengths).astype(np.int32)
    count = lengths.astype(np.int32)
    P = int((lengths + gap).sum())
    if out_of_range:
        P += 5
        start, count = np.append(start, np.int32(P - 5)), np.append(count, np.int32(65))
        if R >= 3:
            start, count = np.append(start, np.int32(-3)), np.append(count, np.int32(10))
    assert start.shape[0] == R
    # three rays in ten are thin (densities x 0.05 or x 0.02: tau averages 0.078 / 0.031), so that a stop also falls into a ray's second,
    # third or fourth chunk, behind one or more carries, or is never reached
    density = rng.random(P) * density_max
    for r, scale in enumerate(rng.choice([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.05, 0.05, 0.02], R)):
        if start[r] >= 0:
            density[int(start[r]):int(start[r]) + int(count[r])] *= scale
    return {"R": R, "P": P, "start": _c(start, np.int32), "count": _c(count, np.int32),
            "density": density.astype(np.float32), "deltas": np.full(P, 1.0 / 64.0, np.float32),
            "t": rng.random(P).astype(np.float32), "xyz": rng.standard_normal((P, 3)).astype(np.float32),
            "dirs": rng.standard_normal((P, 3)).astype(np.float32)}


def rows_of(case, r):
    s, n, P = int(case["start"][r]), int(case["count"][r]), case["P"]
    if s < 0 or s >= P or n <= 0:
        return 0, 0
    return s, min(n, P - s)


def host_count(lib, case, tau_stop, tau_min):
    """the twin's count pass -> (keep (P,) uint8 with 7 in the rows of no ray, new_count (R,))"""
    keep, new_count = np.full(case["P"], 7, np.uint8), np.full(case["R"], -7, np.int32)
    lib.prune_host_count(case["density"].ctypes.data, case["deltas"].ctypes.data, case["start"].ctypes.data, case["count"].ctypes.data, case["R"], case["P"],
                         tau_stop, tau_min, keep.ctypes.data, new_count.ctypes.data)
    return keep, new_count


def host_prune(lib, case, tau_stop, tau_min, cap=None, aabb=AABB):
    """The twin's two passes around numpy's exclusive sum.  cap None: the total.  -> dict with the fields of lab4d_amd.packed.PrunedRays
    (numpy; total an int, overflow a bool), `keep` (zeros in the rows of no ray, as the caller's zero-fill leaves them) and `count`."""
    keep, count = host_count(lib, case, tau_stop, tau_min)
    keep[keep == 7] = 0
    incl = np.cumsum(count, dtype=np.int64)
    start = (incl - count).astype(np.int32)
    if cap is None:
        cap = int(incl[-1]) if case["R"] else 0
    out = {"t": np.full(cap, np.nan, np.float32), "deltas": np.full(cap, np.nan, np.float32), "xyz": np.full((cap, 3), np.nan, np.float32),
           "dirs": np.full((cap, 3), np.nan, np.float32), "ray_idx": np.full(cap, -7, np.int32), "src_row": np.full(cap, -7, np.int32),
           "ray_count": np.full(case["R"], -7, np.int32)}
    total, ovf = np.full(1, -7, np.int32), np.full(1, 7, np.uint8)
    aabb = _c(aabb, np.float32)
    lib.prune_host_write(keep.ctypes.data, case["start"].ctypes.data, case["count"].ctypes.data, start.ctypes.data, case["R"], case["P"], cap, aabb.ctypes.data,
                         case["t"].ctypes.data, case["deltas"].ctypes.data, case["xyz"].ctypes.data, case["dirs"].ctypes.data, out["t"].ctypes.data,
                         out["deltas"].ctypes.data, out["xyz"].ctypes.data, out["dirs"].ctypes.data, out["ray_idx"].ctypes.data, out["src_row"].ctypes.data,
                         out["ray_count"].ctypes.data, total.ctypes.data, ovf.ctypes.data)
    out.update(ray_start=start, total=int(total[0]), overflow=bool(ovf[0]), keep=keep, count=count, R=case["R"], cap=cap)
    return out


def ref_keep(case, tau_stop, tau_min, margin=MARGIN):
    """The rules in float64: (keep (P,) bool, generic (R,) bool, stop (R,) = j* as a place within its ray, -1 where the ray never stops).
    tau = density * delta, NaN or not > 0 -> 0; E = the exclusive prefix sum along the ray; the first row with E > tau_stop and every row
    behind it drop; a row before it is kept iff tau >= tau_min.  A ray is generic when no E lies within `margin` (relative) of tau_stop
    and no tau within `margin` of tau_min."""
    keep, generic, stop_at = np.zeros(case["P"], bool), np.ones(case["R"], bool), np.full(case["R"], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        tau_all = case["density"].astype(np.float64) * case["deltas"].astype(np.float64)
    tau_all = np.where(tau_all > 0, tau_all, 0.0)
    for r in range(case["R"]):
        s, n = rows_of(case, r)
        if n == 0:
            continue
        tau = tau_all[s:s + n]
        E = np.cumsum(tau) - tau
        stop = E > tau_stop
        first = int(np.argmax(stop)) if stop.any() else n
        stop_at[r] = first if stop.any() else -1
        keep[s:s + first] = tau[:first] >= tau_min
        near = False
        if math.isfinite(tau_stop):
            near |= bool((np.abs(E - tau_stop) <= margin * tau_stop).any())
        if tau_min > 0:
            near |= bool((np.abs(tau - tau_min) <= margin * tau_min).any())
        generic[r] = not near
    return keep, generic, stop_at
