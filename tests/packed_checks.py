"""Shared by tests/test_packed_host.py (CPU twin against float64) and tests/test_gpu_zzzzzpacked.py (kernels against the twin): the host
harness of packed marching / compositing (tests/host_harness/packed_host.cpp over lab4d_amd/csrc/packed_math.hpp), the test inputs, and the
rules of include/lab4d_packed.h restated in float64 (numpy for the march; the oracle's compute_weights / integrate with torch autograd for
the compositing).  The grid, ray and occupancy helpers are those of tests/occgrid_checks.py."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import occgrid_checks as OC  # noqa: E402

ROOT = OC.ROOT
FP32_BAR = 1e-4  # the project's fp32 bar (README): max-norm error relative to the reference's max-norm


def build_host():
    return host_twin.load("packed")


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def host_march(lib, origin, direction, t_range, aabb, bits, G, dt, k_max, cap=None):
    """The twin's two passes around numpy's exclusive sum.  cap None: the total (nothing dropped).  Returns a dict with the fields of
    lab4d_amd.packed.PackedRays (numpy; total an int, overflow a bool) and `count`, the untruncated per-ray counts."""
    origin, direction, t_range, aabb = (_c(a, np.float32) for a in (origin, direction, t_range, aabb))
    bits = _c(bits, np.uint32)
    R = origin.shape[0]
    count = np.zeros(R, np.int32)
    head = (origin.ctypes.data, direction.ctypes.data, t_range.ctypes.data, aabb.ctypes.data, bits.ctypes.data, G, R, dt, k_max)
    lib.packed_host_march_count(*head, count.ctypes.data)
    incl = np.cumsum(count, dtype=np.int64)
    start = (incl - count).astype(np.int32)
    if cap is None:
        cap = int(incl[-1]) if R else 0
    out = {"t": np.full(cap, np.nan, np.float32), "deltas": np.full(cap, np.nan, np.float32), "xyz": np.full((cap, 3), np.nan, np.float32),
           "dirs": np.full((cap, 3), np.nan, np.float32), "ray_idx": np.full(cap, -7, np.int32), "ray_count": np.full(R, -7, np.int32)}
    total, ovf = np.full(1, -7, np.int32), np.full(1, 7, np.uint8)
    lib.packed_host_march_write(*head, start.ctypes.data, cap, out["t"].ctypes.data, out["deltas"].ctypes.data, out["xyz"].ctypes.data, out["dirs"].ctypes.data,
                                out["ray_idx"].ctypes.data, out["ray_count"].ctypes.data, total.ctypes.data, ovf.ctypes.data)
    out.update(ray_start=start, total=int(total[0]), overflow=bool(ovf[0]), count=count, R=R, cap=cap)
    return out


def _field_args(fields, modes):
    fields = [_c(f, np.float32) for f in fields]
    n = len(fields)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[f.ctypes.data for f in fields])
    chans = (ctypes.c_int * max(n, 1))(*[f.shape[1] for f in fields])
    ms = (ctypes.c_int * max(n, 1))(*modes)
    return fields, n, ptrs, chans, ms, sum(1 if m == 2 else f.shape[1] for f, m in zip(fields, modes))


def host_composite(lib, density, deltas, fields, modes, start, count, g_mask=None, g_out=None):
    """The twin's forward and (with g_mask / g_out) backward: dict with weights, transmit, mask (R,), out (R, sumC), and the gradients
    g_density, g_deltas, g_fields (zeros in the rows that no ray owns)."""
    density, deltas = _c(density, np.float32), _c(deltas, np.float32)
    start, count = _c(start, np.int32), _c(count, np.int32)
    fields, n, ptrs, chans, ms, sumC = _field_args(fields, modes)
    P, R = density.shape[0], start.shape[0]
    res = {"weights": np.zeros(P, np.float32), "transmit": np.zeros(P, np.float32), "mask": np.full(R, np.nan, np.float32),
           "out": np.full((R, sumC), np.nan, np.float32)}
    lib.packed_host_composite_forward(density.ctypes.data, deltas.ctypes.data, n, ptrs, chans, ms, start.ctypes.data, count.ctypes.data, R, P,
                                      res["weights"].ctypes.data, res["transmit"].ctypes.data, res["mask"].ctypes.data, res["out"].ctypes.data)
    if g_mask is not None:
        g_mask, g_out = _c(g_mask, np.float32), _c(g_out, np.float32)
        res["g_density"], res["g_deltas"] = np.zeros(P, np.float32), np.zeros(P, np.float32)
        res["g_fields"] = [np.zeros_like(f) for f in fields]
        gptrs = (ctypes.c_void_p * max(n, 1))(*[g.ctypes.data for g in res["g_fields"]])
        lib.packed_host_composite_backward(density.ctypes.data, deltas.ctypes.data, n, ptrs, chans, ms, start.ctypes.data, count.ctypes.data, R, P,
                                           g_mask.ctypes.data, g_out.ctypes.data, res["g_density"].ctypes.data, res["g_deltas"].ctypes.data, gptrs)
    return res


# ---------------------------------------------------------------------------------------------------
# the march in float64
# ---------------------------------------------------------------------------------------------------
def lattice(t_range, dt, k_max):
    """t_k (R, k_max) float32, formed as the rule says (every product and sum rounded to float32), and valid (R, k_max): t_k <= t1"""
    with np.errstate(invalid="ignore", over="ignore"):
        step = (np.arange(k_max, dtype=np.float32) + np.float32(0.5)) * np.float32(dt)
        tk = (t_range[:, :1].astype(np.float32) + step[None, :]).astype(np.float32)
        return tk, tk <= t_range[:, 1:2]


def ref_march(origin, direction, t_range, occ, G, dt, k_max, aabb=OC.AABB):
    """(tk (R,K) f32, candidate (R,K), keep (R,K), clear (R,K)): candidate = t_k <= t1 on a ray with finite inputs and t0 <= t1; keep = the
    float64 point o + t_k d lies in an occupied cell; clear = it is farther than OC.MARGIN cell edges from every cell face on all three axes"""
    tk, valid = lattice(t_range, dt, k_max)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(origin).all(1) & np.isfinite(direction).all(1) & np.isfinite(t_range).all(1) & (t_range[:, 0] <= t_range[:, 1])
    cand = valid & ok[:, None]
    R, K = tk.shape
    o, d = np.nan_to_num(origin.astype(np.float64)), np.nan_to_num(direction.astype(np.float64))
    p = o[:, None, :] + np.nan_to_num(tk.astype(np.float64))[:, :, None] * d[:, None, :]
    has, cell, clear = OC.ref_cells(OC.x01_f64(p.reshape(-1, 3), aabb), G)
    keep = (has & occ[cell[:, 0], cell[:, 1], cell[:, 2]]).reshape(R, K) & cand
    return tk, cand, keep, clear.reshape(R, K)


def kept_matrix(res, tk, t_range, dt):
    """The twin's (or the kernels') kept samples as a boolean (R, K) matrix: every kept t must BE a lattice value of its ray"""
    kept = np.zeros(tk.shape, bool)
    n = min(res["total"], res["cap"])
    r, t = res["ray_idx"][:n].astype(np.int64), res["t"][:n]
    k = np.rint((t.astype(np.float64) - t_range[r, 0]) / dt - 0.5).astype(np.int64)
    assert ((k >= 0) & (k < tk.shape[1])).all()
    assert np.array_equal(tk[r, k], t), "a kept t is not a value of its ray's lattice"
    kept[r, k] = True
    assert kept.sum() == n, "a lattice value was emitted twice"
    return kept


def outside_rays(n, seed, aabb=OC.AABB):
    """generic rays: random origins outside the box (0.9 .. 1.1 box edges from its centre), random directions through a random point of the
    box, of length 0.5 .. 2 box edges (t is not a distance); t0 in [0, 0.2], t1 in [3, 6]"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    o = 0.5 + u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))
    d = (rng.uniform(0.02, 0.98, (n, 3)) - o) * rng.uniform(0.5, 2.0, (n, 1))
    lo, ext = aabb[0].astype(np.float64), aabb[1].astype(np.float64) - aabb[0]
    t = np.stack([rng.uniform(0.0, 0.2, n), rng.uniform(3.0, 6.0, n)], 1)
    return (lo + o * ext).astype(np.float32), (d * ext).astype(np.float32), t.astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 63, 64, 65, 129)


def composite_case(channels, modes, seed, lengths=LENGTHS, gap=3):
    """A packed list whose rays have the given lengths, `gap` rows that no ray owns behind the last one; tau = density * delta averages
    0.08, so a ray of 129 samples ends at a transmittance of e^-10 and every sample still counts.  Returns numpy float32 / int32 arrays."""
    rng = np.random.default_rng(seed)
    count = np.array(lengths, np.int32)
    start = (np.cumsum(count) - count).astype(np.int32)
    P = int(count.sum()) + gap
    case = {"density": (rng.random(P) * 8).astype(np.float32), "deltas": (0.01 + 0.02 * rng.random(P)).astype(np.float32),
            "fields": [rng.standard_normal((P, c)).astype(np.float32) for c in channels], "modes": list(modes), "start": start, "count": count,
            "P": P, "R": len(lengths)}
    sumC = sum(1 if m == 2 else c for c, m in zip(channels, modes))
    case["g_mask"] = rng.standard_normal(case["R"]).astype(np.float32)
    case["g_out"] = rng.standard_normal((case["R"], sumC)).astype(np.float32)
    return case


_FREEZE = ("cyc_dist", "xyz_cam", "skin_entropy")  # the oracle's detached-weight keys


def ref_composite(case):
    """float64: oracle.lab4d_oracle.compute_weights + integrate ray by ray at D = the ray's count (a mode-2 field is render_pixel's plain
    mean; a ray without samples renders zeros, as the contract says), and torch autograd of sum(g_mask * mask) + sum(g_out * out) for the
    gradients.  Returns numpy float64: mask, out, weights, transmit, g_density, g_deltas, g_fields."""
    import torch
    sys.path.insert(0, ROOT)
    from oracle import lab4d_oracle as LO
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    density, deltas = t64(case["density"]), t64(case["deltas"])
    fields = [t64(f) for f in case["fields"]]
    masks, outs = [], []
    weights, transmit = np.zeros(case["P"]), np.zeros(case["P"])
    for s, n in zip(case["start"], case["count"]):
        s, n = int(s), int(n)
        if n == 0:
            masks.append(torch.zeros(1, dtype=torch.float64))
            outs.append(torch.zeros(case["g_out"].shape[1], dtype=torch.float64))
            continue
        w, T = LO.compute_weights(density[s:s + n].reshape(1, 1, n, 1), deltas[s:s + n].reshape(1, 1, n, 1))
        weights[s:s + n], transmit[s:s + n] = w.detach().numpy().reshape(-1), T.detach().numpy().reshape(-1)
        fd, keys = {"density_any": torch.ones(1, 1, n, 1, dtype=torch.float64)}, []  # (integrate needs one density_ key to normalise)
        for i, (f, m) in enumerate(zip(fields, case["modes"])):
            keys.append(None if m == 2 else (_FREEZE[i] if m == 1 else "field%d" % i))
            if m != 2:
                fd[keys[-1]] = f[s:s + n].reshape(1, 1, n, -1)
        res = LO.integrate(fd, w)
        masks.append(res["mask"].reshape(1))
        outs.append(torch.cat([f[s:s + n].mean().reshape(1) if k is None else res[k].reshape(-1) for f, k in zip(fields, keys)]
                              or [torch.zeros(0, dtype=torch.float64)]))
    mask, out = torch.cat(masks), torch.stack(outs)
    loss = (mask * torch.tensor(case["g_mask"].astype(np.float64))).sum() + (out * torch.tensor(case["g_out"].astype(np.float64))).sum()
    grads = torch.autograd.grad(loss, [density, deltas] + fields, allow_unused=True)
    g = [np.zeros(tuple(x.shape)) if gr is None else gr.numpy() for gr, x in zip(grads, [density, deltas] + fields)]
    return {"mask": mask.detach().numpy(), "out": out.detach().numpy(), "weights": weights, "transmit": transmit, "g_density": g[0], "g_deltas": g[1],
            "g_fields": g[2:]}


def rel_max(a, b):
    """max-norm error relative to the reference's max-norm (two all-zero arrays: 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def check_composite(got, ref, what=""):
    """got: float32 results (the twin's or the kernels'), ref: ref_composite's; everything within FP32_BAR and free of NaN"""
    errs = {k: rel_max(got[k], ref[k]) for k in ("mask", "out", "weights", "transmit", "g_density", "g_deltas") if k in got}
    for i, (g, r) in enumerate(zip(got.get("g_fields", []), ref["g_fields"])):
        errs["g_field%d" % i] = rel_max(g, r)
    print("composite %s:" % what, {k: "%.2e" % v for k, v in errs.items()})
    for k, v in errs.items():
        assert v < FP32_BAR, (what, k, v)
    for k in ("mask", "out", "g_density", "g_deltas"):
        if k in got:
            assert np.isfinite(got[k]).all(), (what, k)
