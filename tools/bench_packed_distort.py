"""The distortion loss of the packed sample list, measured: the chunk of tools/bench_packed.py (one chunk of `bench.py --config hash`, 2 x 16
rows x 1024 rays x 256 candidates, the ball-shaped field of tools/bench_occgrid.py behind a G = 128 occupancy grid), marched once; the
density of the kept rows comes from hashfield.density.  Two paths to the same per-ray loss, alternating in one process:
    library  lab4d_packed_distortion_forward / _backward (include/lab4d_distort.h) on buffers allocated once
    padded   torch ops on an (R, max_count) pad gathered from the packed list: tau, its exclusive cumsum, w, the prefix sums of w and w m,
             the row terms and their sum, and autograd for the adjoint (max_count is read back once, outside the timed region)
Times are device-event medians of 5 repetitions after a warm-up of every shape.  The kernels' achieved bytes per second are reported against
what they must move: 16 B per owned row forward (density, deltas, mid, width), 24 B (one gradient) to 28 B (both) per owned row for the
adjoint, whose second sweep over the same rows is not counted.  The chunk's list is small (its launches sit at the launch floor), so the
library's calls are also timed on a dense list of --dense-rays x --dense-rows rows.  No number here is asserted anywhere and no ratio is
promised.

    python tools/bench_packed_distort.py [--out profiles/packed_distort.json] [--res 1024] [--spp 256] [--rows 16] [--dense-rays 131072] [--dense-rows 128]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_occgrid import ball_tables, clock_state, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_distort.json"))
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--G", type=int, default=128)
    ap.add_argument("--dense-rays", type=int, default=131072)
    ap.add_argument("--dense-rows", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_packed_distort.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, hashfield, mlp, occgrid, packed, synthetic
    from lab4d_amd import quat_utils as Q, render_utils as RU
    _lib.lib()
    clocks = {"before": clock_state()}
    fr = synthetic.to_device(synthetic.make_frames(1, 2, a.res), dev)
    cam2field = Q.quaternion_translation_inverse(fr["field2cam"][0], fr["field2cam"][1])
    n_chunks = a.res // a.rows
    K = a.spp
    with torch.no_grad():
        hxy = synthetic.make_rays(a.res, 2, rows=list(range(a.res))[0::n_chunks]).to(dev)
        out = RU.ray_samples(hxy, fr["Kinv"], fr["near_far"], cam2field, n_depth=2)  # two depths per ray: the ray's origin and direction in the field's frame
        x, depth = out[4].reshape(-1, 2, 3), out[3].reshape(-1, 2, 1)
        d = ((x[:, 1] - x[:, 0]) / (depth[:, 1] - depth[:, 0])).contiguous()  # per unit of depth
        o = (x[:, 0] - depth[:, 0] * d).contiguous()
        R = o.shape[0]
        nf = fr["near_far"][:, None, :].expand(2, R // 2, 2).reshape(R, 2).contiguous()
    dt = float((nf[:, 1] - nf[:, 0]).max()) / K
    P, cfg = hashfield.make_weights(0, sdf_bias=0.02)
    ball_tables(P, cfg)
    P = synthetic.to_device(P, dev)
    grid = hashfield.update_occupancy(P, cfg, occgrid.OccupancyGrid(P["aabb"], G=a.G), prec=mlp.PREC_BF16)
    with torch.no_grad():
        marched = int(packed.march(grid, o, d, nf, dt, 0, k_max=K).total)
        cap = (int(1.25 * marched) + 1023) // 1024 * 1024
        rays = packed.march(grid, o, d, nf, dt, cap, k_max=K)
        density = hashfield.density(P, cfg, rays.xyz, mlp.PREC_BF16).reshape(-1).contiguous()
        deltas, width = rays.deltas, rays.deltas
        mid = (rays.t * rays.deltas / dt).contiguous()
        max_count = int(rays.ray_count.max())  # (the pad's width: a read-back, once)
        n_hit = int((rays.ray_count > 0).sum())
    g_loss = torch.full((R,), 1.0 / R, device=dev)
    loss = torch.empty(R, device=dev)
    g_density, g_deltas = torch.zeros(cap, device=dev), torch.zeros(cap, device=dev)
    head = [density, deltas, mid, width, rays.ray_start, rays.ray_count, R, cap]

    def lib_forward():
        _lib.call("packed_distortion_forward", *head, loss)

    def lib_backward(both=True):
        _lib.call("packed_distortion_backward", *head, g_loss, g_density, g_deltas if both else None)

    def lib_autograd():
        dn, dl = density.clone().requires_grad_(True), deltas.clone().requires_grad_(True)
        packed.distortion(dn, dl, mid, width, rays).mean().backward()
        return dn.grad, dl.grad

    def padded(dn, dl):
        j = torch.arange(max_count, device=dev)
        valid = j[None, :] < rays.ray_count[:, None]
        rows = (rays.ray_start[:, None].long() + j[None, :]).clamp_(max=cap - 1)
        tau = torch.where(valid, dn[rows] * dl[rows], 0.0)
        w = (1 - torch.exp(-tau)) * torch.exp(-(torch.cumsum(tau, 1) - tau))
        m = torch.where(valid, mid[rows] - mid[rows[:, :1]], 0.0)
        wm = w * m
        return (2 * w * (m * (torch.cumsum(w, 1) - w) - (torch.cumsum(wm, 1) - wm)) + w * w * torch.where(valid, width[rows], 0.0) / 3).sum(1)

    def pad_forward():
        with torch.no_grad():
            return padded(density, deltas)

    def pad_autograd():
        dn, dl = density.clone().requires_grad_(True), deltas.clone().requires_grad_(True)
        padded(dn, dl).mean().backward()
        return dn.grad, dl.grad

    paths = {"library forward": lib_forward, "padded forward": pad_forward, "library forward + backward (autograd)": lib_autograd,
             "padded forward + backward (autograd)": pad_autograd, "library backward, both gradients": lib_backward,
             "library backward, g_density alone": lambda: lib_backward(False)}
    for fn in paths.values():  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    lib_forward()
    ref = pad_forward()
    (ga, gb), (pa, pb) = lib_autograd(), pad_autograd()
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))
    agree = {"loss": rel(loss, ref), "g_density": rel(ga, pa), "g_deltas": rel(gb, pb)}
    t = {k: [] for k in paths}
    for _ in range(5):  # alternating, so that a drifting clock hits all alike
        for name, fn in paths.items():
            t[name].append(timed(fn, reps=1)["median_ms"])
    stat = lambda v: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    times = {k: stat(v) for k, v in t.items()}
    owned = min(marched, cap)
    gbs = lambda bytes_per_row, k: round(owned * bytes_per_row / (times[k]["median_ms"] * 1e-3) / 1e9, 1)
    result = {
        "workload": "distortion loss of one marched chunk of the hash configuration: %d rays x %d candidates, ball field, G = %d, "
                    "density from hashfield.density (bf16 chains)" % (R, K, a.G),
        "dt": dt, "rays": R, "rays_with_rows": n_hit, "marched_rows": marched, "capacity": cap, "max_count": max_count, "padded_elements": R * max_count,
        "loss_mean": float(loss.mean()), "rel_max_library_vs_padded": agree,
        "times": times,
        "ratio_of_medians_padded_over_library": {
            "forward": round(times["padded forward"]["median_ms"] / times["library forward"]["median_ms"], 2),
            "forward + backward (autograd)": round(times["padded forward + backward (autograd)"]["median_ms"]
                                                   / times["library forward + backward (autograd)"]["median_ms"], 2)},
        "achieved_GB_per_s": {"forward, 16 B per owned row": gbs(16, "library forward"),
                              "backward with both gradients, 28 B per owned row": gbs(28, "library backward, both gradients"),
                              "backward with g_density alone, 24 B per owned row": gbs(24, "library backward, g_density alone")},
    }
    # The chunk's 82 k rows are 1.3 MB: its launches measure the launch floor, not the memory system.  A list large enough to show what the
    # kernels sustain: --dense-rays rays of --dense-rows rows back to back, composite-shaped values (tau averages 0.08), the library's calls alone.
    Rd, n = a.dense_rays, a.dense_rows
    Pd = Rd * n
    g = torch.Generator(device=dev).manual_seed(1)
    dn, dl = torch.rand(Pd, device=dev, generator=g) * 8, 0.01 + 0.02 * torch.rand(Pd, device=dev, generator=g)
    md = (torch.cumsum(dl.view(Rd, n), 1) - 0.5 * dl.view(Rd, n)).reshape(Pd).contiguous()
    start = torch.arange(Rd, device=dev, dtype=torch.int32) * n
    count = torch.full((Rd,), n, device=dev, dtype=torch.int32)
    out_d, go_d, gd_d, gl_d = torch.empty(Rd, device=dev), torch.full((Rd,), 1.0 / Rd, device=dev), torch.zeros(Pd, device=dev), torch.zeros(Pd, device=dev)
    dense = {"forward": lambda: _lib.call("packed_distortion_forward", dn, dl, md, dl, start, count, Rd, Pd, out_d),
             "backward, both gradients": lambda: _lib.call("packed_distortion_backward", dn, dl, md, dl, start, count, Rd, Pd, go_d, gd_d, gl_d),
             "backward, g_density alone": lambda: _lib.call("packed_distortion_backward", dn, dl, md, dl, start, count, Rd, Pd, go_d, gd_d, None)}
    for fn in dense.values():
        fn()
    torch.cuda.synchronize()
    td = {k: [] for k in dense}
    for _ in range(5):
        for name, fn in dense.items():
            td[name].append(timed(fn, reps=1)["median_ms"])
    result["dense_list"] = {"rays": Rd, "rows_per_ray": n, "rows": Pd, "times": {k: stat(v) for k, v in td.items()},
                            "achieved_GB_per_s": {k: round(Pd * b / (statistics.median(td[k]) * 1e-3) / 1e9, 1)
                                                  for k, b in (("forward", 16), ("backward, both gradients", 28), ("backward, g_density alone", 24))}}
    clocks["after"] = clock_state()
    result["clock_state"] = clocks
    result["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
