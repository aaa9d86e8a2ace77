"""Pruning of the packed sample list, measured: the chunk of tools/bench_packed.py (one chunk of `bench.py --config hash`, 2 x 16 rows x 1024
rays, the ball-shaped field of tools/bench_occgrid.py behind a G = 128 occupancy grid, bf16 chains, packed-fp16 table gradient) with the
ball made OPAQUE (1 / beta = --ibeta, the density inside the ball), so that a ray's transmittance falls below early_stop_eps inside the ball.
Two paths, alternating in one process:
    packed  hashfield.render_packed: packed.march, the field on all kept rows, packed.composite
    pruned  hashfield.render_packed_pruned: the same march, hashfield.density without gradients, packed.prune, the field on the survivors
Forward + backward of each, the two prune launches alone (the library's calls on buffers allocated once), the marched and the kept totals
and the share of rays that reach the stop.  Times are device-event medians of 5 repetitions after a warm-up of every shape; no number here
is asserted anywhere and no ratio is promised.

    python tools/bench_packed_prune.py [--out profiles/packed_prune.json] [--res 1024] [--spp 256] [--rows 16] [--ibeta 400] [--eps 1e-4]
"""
import argparse
import json
import math
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_prune.json"))
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--G", type=int, default=128)
    ap.add_argument("--ibeta", type=float, default=400.0)
    ap.add_argument("--eps", type=float, default=1e-4)
    ap.add_argument("--alpha", type=float, default=0.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_packed_prune.py measures on the GPU; none found (there is no CPU path)")
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
    P["logibeta"] = torch.tensor([math.log(a.ibeta)])
    P = synthetic.to_device(P, dev)
    params = [v for k, v in P.items() if k != "aabb"]
    for v in params:
        v.requires_grad_(True)
    hres = hashfield.resolutions(cfg, dev)
    grid = hashfield.update_occupancy(P, cfg, occgrid.OccupancyGrid(P["aabb"], G=a.G), prec=mlp.PREC_BF16)
    with torch.no_grad():
        marched = int(packed.march(grid, o, d, nf, dt, 0, k_max=K).total)
    cap = (int(1.25 * marched) + 1023) // 1024 * 1024
    with torch.no_grad():
        rays = packed.march(grid, o, d, nf, dt, cap, k_max=K)
        dens = hashfield.density(P, cfg, rays.xyz, mlp.PREC_BF16, res=hres)
        pruned = packed.prune(rays, dens, early_stop_eps=a.eps, alpha_thre=a.alpha, aabb=grid.aabb)
        kept = int(pruned.total)
        hit = rays.ray_count > 0
        # a ray reaches the stop when rows of it are dropped although every row passes the opacity rule (alpha = 0), else: an upper bound
        stopped = int(((pruned.ray_count < rays.ray_count) & hit).sum())
        n_hit = int(hit.sum())
    prune_cap = (int(1.25 * kept) + 1023) // 1024 * 1024
    ovf = torch.zeros(1, dtype=torch.bool, device=dev)

    def packed_path(backward=True):
        rgb, mask, depth_r, _, ov = hashfield.render_packed(P, cfg, grid, o, d, nf, dt, cap, prec=mlp.PREC_BF16, table_grad_f16=True, k_max=K, res=hres)
        ovf.logical_or_(ov)
        if backward:
            (rgb.mean() + mask.mean() + depth_r.mean()).backward()
            for v in params:
                v.grad = None
        return rgb, mask, depth_r

    def pruned_path(backward=True):
        rgb, mask, depth_r, _, ov, _, kov = hashfield.render_packed_pruned(P, cfg, grid, o, d, nf, dt, cap, prec=mlp.PREC_BF16, table_grad_f16=True, k_max=K,
                                                                           res=hres, early_stop_eps=a.eps, alpha_thre=a.alpha, prune_cap=prune_cap)
        ovf.logical_or_(ov | kov)
        if backward:
            (rgb.mean() + mask.mean() + depth_r.mean()).backward()
            for v in params:
                v.grad = None
        return rgb, mask, depth_r

    paths = {"packed": packed_path, "pruned": pruned_path}
    for fn in paths.values():  # warm-up of both shapes
        fn()
    torch.cuda.synchronize()
    with torch.no_grad():
        a_, b_ = packed_path(False), pruned_path(False)
        agree = {k: float((x - y).abs().max()) for k, x, y in zip(("rgb", "mask", "depth"), b_, a_)}
    t = {k: [] for k in paths}
    for _ in range(5):  # alternating, so that a drifting clock hits both alike
        for name, fn in paths.items():
            t[name].append(timed(fn, reps=1)["median_ms"])
    assert not bool(ovf), "a packed buffer overflowed: samples were dropped"
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    # the two prune launches alone: the library's calls on buffers allocated once (no cumsum, no fills, no allocations)
    tau_stop, tau_min = packed.prune_thresholds(a.eps, a.alpha)
    dens1 = dens.reshape(-1).contiguous()
    keep = torch.zeros(cap, dtype=torch.uint8, device=dev)
    cnt = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call("packed_prune_count", dens1, rays.deltas, rays.ray_start, rays.ray_count, R, cap, tau_stop, tau_min, keep, cnt)
    start = torch.cumsum(cnt, 0, dtype=torch.int32) - cnt
    ob = {"t": torch.empty(prune_cap, device=dev), "deltas": torch.empty(prune_cap, device=dev), "xyz": torch.empty(prune_cap, 3, device=dev),
          "dirs": torch.empty(prune_cap, 3, device=dev), "ray_idx": torch.empty(prune_cap, dtype=torch.int32, device=dev),
          "src_row": torch.empty(prune_cap, dtype=torch.int32, device=dev)}
    cnt_out, tot, ov8 = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.uint8, device=dev)

    def prune_count():
        _lib.call("packed_prune_count", dens1, rays.deltas, rays.ray_start, rays.ray_count, R, cap, tau_stop, tau_min, keep, cnt)

    def prune_write():
        _lib.call("packed_prune_write", keep, rays.ray_start, rays.ray_count, start, R, cap, prune_cap, grid.aabb, rays.t, rays.deltas, rays.xyz, rays.dirs,
                  ob["t"], ob["deltas"], ob["xyz"], ob["dirs"], ob["ray_idx"], ob["src_row"], cnt_out, tot, ov8)

    def density_pass():
        with torch.no_grad():
            hashfield.density(P, cfg, rays.xyz, mlp.PREC_BF16, res=hres)

    result = {
        "workload": "forward + backward of one chunk of the hash configuration: %d rays x %d candidates, opaque ball field (1 / beta = %g), bf16 chains, "
                    "packed-fp16 table gradient, G = %d, early_stop_eps = %g, alpha_thre = %g" % (R, K, a.ibeta, a.G, a.eps, a.alpha),
        "dt": dt, "marched_rows": marched, "kept_rows": kept, "kept_fraction_of_marched": round(kept / max(marched, 1), 4),
        "rays": R, "rays_with_rows": n_hit, "rays_that_reach_the_stop": stopped, "share_of_rays_with_rows_that_reach_the_stop": round(stopped / max(n_hit, 1), 4),
        "capacity": cap, "prune_capacity": prune_cap,
        "render_packed": stat(t["packed"]), "render_packed_pruned": stat(t["pruned"]),
        "ratio_of_medians_packed_over_pruned": round(statistics.median(t["packed"]) / statistics.median(t["pruned"]), 3),
        "max_abs_difference_pruned_vs_packed": agree,
        "kernels": {
            "prune count (%d rays, %d rows)" % (R, cap): timed(prune_count),
            "prune write + park (%d survivors into %d rows)" % (kept, prune_cap): timed(prune_write),
            "packed.prune (both launches, the scan, the fills and allocations)": timed(lambda: packed.prune(rays, dens, early_stop_eps=a.eps, alpha_thre=a.alpha,
                                                                                                           cap=prune_cap, aabb=grid.aabb)),
            "hashfield.density without gradients (%d rows)" % cap: timed(density_pass),
        },
    }
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
