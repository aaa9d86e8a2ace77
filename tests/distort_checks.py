"""Shared by tests/test_distort_host.py (CPU twin against float64) and tests/test_gpu_zzzzzzzzzdistort.py (kernels against float64 and the
twin): the host harness of the distortion loss (tests/host_harness/distort/distort_host.cpp over lab4d_amd/csrc/distort_math.hpp), the test
lists -- the committed generators of tests/packed_checks.py and tests/prune_checks.py with midpoints and widths added -- and the rule of
include/lab4d_distort.h as its DEFINITION in torch float64: the O(n^2) double sum per ray, with autograd.  A helper module: no test in it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import packed_checks as PC  # noqa: E402
import prune_checks as PR  # noqa: E402

FP32_BAR = PC.FP32_BAR
rel_max = PC.rel_max
rows_of = PR.rows_of
TWIN = "distort/distort"  # tests/host_harness/distort/distort_host.cpp: a folder of its own (tests/test_host_twin.py pins the census of the twins beside it)
MID_OFFSET = 3.0
OUTPUTS = ("loss", "g_density", "g_deltas")


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def groups(case):
    """the rays with rows, by length: (ray numbers (k,), rows (k, n)) per distinct n > 0, each ray cut to [0, P) by the rule of the header"""
    sn = np.array([rows_of(case, r) for r in range(case["R"])], np.int64).reshape(-1, 2)
    for n in np.unique(sn[:, 1]):
        if n > 0:
            rays = np.flatnonzero(sn[:, 1] == n)
            yield rays, sn[rays, :1] + np.arange(n)[None, :]


def add_intervals(case, seed):
    """width = the row's deltas; mid = the cumulative midpoint of width along the ray, started at MID_OFFSET (so that the shift by the
    ray's first midpoint is exercised); a third of the rays have random gaps of up to two widths between their intervals.  Formed in
    float64, rounded to float32 once.  Rows of no ray: width 0, mid 0.  A g_loss (R,) comes with it."""
    rng = np.random.default_rng(seed)
    width = np.zeros(case["P"], np.float64)
    mid = np.zeros(case["P"], np.float64)
    for rays, rows in groups(case):
        w = case["deltas"][rows].astype(np.float64)
        gap = rng.random(rows.shape) * 2 * w * (rng.integers(0, 3, (len(rays), 1)) == 0)
        width[rows] = w
        mid[rows] = MID_OFFSET + np.cumsum(w + gap, 1) - 0.5 * w
    case.update(width=width.astype(np.float32), mid=mid.astype(np.float32), g_loss=rng.standard_normal(case["R"]).astype(np.float32))
    return case


def composite_list(seed):
    """packed_checks.composite_case: lengths 0 / 1 / 2 / 63 / 64 / 65 / 129, 3 unowned rows behind, density in [0, 8], deltas 0.01 .. 0.03"""
    c = PC.composite_case([], [], seed)
    return add_intervals({k: c[k] for k in ("R", "P", "start", "count", "density", "deltas")}, seed + 1000)


def ragged_list(R, seed):
    """prune_checks.make_list: lengths up to 200, gaps of unowned rows, a (start, count) that leaves [0, P) at either end, deltas 1/64,
    density in [0, 200]"""
    c = PR.make_list(R, seed)
    return add_intervals({k: c[k] for k in ("R", "P", "start", "count", "density", "deltas")}, seed + 1000)


def short_rays(R, seed):
    """many short rays (0 / 1 / 2 / 3 rows, one in a hundred 70), back to back, in the ragged list's units"""
    rng = np.random.default_rng(seed)
    count = rng.choice(np.int32([0, 1, 2, 3, 70]), R, p=[0.3, 0.3, 0.2, 0.19, 0.01])
    P = int(count.sum())
    case = {"R": R, "P": P, "start": (np.cumsum(count) - count).astype(np.int32), "count": count,
            "density": (rng.random(P) * 200).astype(np.float32), "deltas": np.full(P, 1 / 64, np.float32)}
    return add_intervals(case, seed + 1000)


def poisoned(case):
    """the case with NaN in every input row that no ray owns"""
    owned = np.zeros(case["P"], bool)
    for _, rows in groups(case):
        owned[rows] = True
    out = dict(case)
    for k in ("density", "deltas", "mid", "width"):
        out[k] = np.where(owned, case[k], np.float32(np.nan)).astype(np.float32)
    out["owned"] = owned
    return out


def ref_distortion(case):
    """The definition in torch float64 on the float32 inputs: per ray  sum_i sum_j w_i w_j |mid_i - mid_j| + (1/3) sum_i w_i^2 width_i,
    w_i = (1 - exp(-tau_i)) exp(-sum_{j<i} tau_j), tau = density * deltas, as a (k, n, n) pair matrix per group of k rays of n rows; the
    gradients are autograd's of sum(g_loss * loss).  Only rows that a ray owns are read.  -> numpy float64: loss (R,), g_density, g_deltas
    (P,) with zeros in the rows of no ray."""
    import torch
    density = torch.tensor(case["density"].astype(np.float64), requires_grad=True)
    deltas = torch.tensor(case["deltas"].astype(np.float64), requires_grad=True)
    mid, width = torch.tensor(case["mid"].astype(np.float64)), torch.tensor(case["width"].astype(np.float64))
    g_loss = torch.tensor(case["g_loss"].astype(np.float64))
    loss = torch.zeros(case["R"], dtype=torch.float64)
    for rays, rows in groups(case):
        rays, rows = torch.from_numpy(rays), torch.from_numpy(rows)
        tau = density[rows] * deltas[rows]
        w = (1 - torch.exp(-tau)) * torch.exp(-(torch.cumsum(tau, 1) - tau))
        m = mid[rows]
        pair = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2))
        loss = loss.index_add(0, rays, pair + (w * w * width[rows]).sum(1) / 3)
    out = {"loss": loss.detach().numpy(), "g_density": np.zeros(case["P"]), "g_deltas": np.zeros(case["P"])}
    if loss.requires_grad:
        gd, gl = torch.autograd.grad((loss * g_loss).sum(), [density, deltas])
        out.update(g_density=gd.numpy(), g_deltas=gl.numpy())
    return out


def host_distortion(lib, case, which=("g_density", "g_deltas"), sentinel=0.0):
    """the twin's forward and backward: loss (R,) and the gradients named in `which` (P,), `sentinel` in the rows of no ray"""
    c = {k: np.ascontiguousarray(case[k]) for k in ("density", "deltas", "mid", "width", "start", "count", "g_loss")}
    head = [c[k].ctypes.data if c[k].size else None for k in ("density", "deltas", "mid", "width", "start", "count")] + [case["R"], case["P"]]
    out = {"loss": np.full(case["R"], np.nan, np.float32)}
    lib.distort_host_forward(*head, out["loss"].ctypes.data if case["R"] else None)
    for k in which:
        out[k] = np.full(case["P"], sentinel, np.float32)
    lib.distort_host_backward(*head, c["g_loss"].ctypes.data if case["R"] else None, *[out[k].ctypes.data if k in out and case["P"] else None for k in OUTPUTS[1:]])
    return out


def errors(got, ref):
    return {k: rel_max(got[k], ref[k]) for k in OUTPUTS if k in got}


def check(got, ref, what):
    """every output that `got` has, within FP32_BAR of the reference in rel_max (the figures are printed first) and free of NaN"""
    errs = errors(got, ref)
    print("distortion %s:" % (what,), {k: "%.2e" % v for k, v in errs.items()})
    for k, v in errs.items():
        assert np.isfinite(got[k]).all(), (what, k)
        assert v < FP32_BAR, (what, k, v)
    return errs
