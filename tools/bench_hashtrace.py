"""Surface rendering by sphere tracing, measured: the chunk of tools/bench_packed.py (one chunk of `bench.py --config hash`, 2 x 16 rows x 1024
rays, the ball-shaped field of tools/bench_occgrid.py behind a G = 128 occupancy grid, bf16 chains) with the ball made opaque as in
tools/bench_packed_prune.py.  Two paths under no_grad, on the same rays and the same grid, alternating in one process:
    surface  hashfield.render_surface: grid.ray_span, ONE trace launch, sdf_gradient and forward on one row per ray
    pruned   hashfield.render_packed_pruned: packed.march, hashfield.density, packed.prune, forward on the survivors, packed.composite
and the trace kernel alone (the library's call on buffers allocated once).  The ball field's sdf is NOT metric: it is 1 - relu(20 (0.3 - r01)),
83 times the distance in world units near its surface, so the tracer runs with step_scale = (hi - lo) / 20 (a step of the metric distance) and
eps in the field's own units.  Times are device-event medians of 5 repetitions after a warm-up of every shape; the tracer's mean and maximum
n_eval, its status histogram, what the divergent trip counts cost (n_eval summed over the lanes of a wave against 64 x the wave's maximum), the
depth difference between the two renderings and the clock state go into the file.  No number here is asserted anywhere and no ratio is promised.

    python tools/bench_hashtrace.py [--out profiles/hashtrace.json] [--res 1024] [--spp 256] [--rows 16] [--ibeta 400] [--eps 0.01]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hashtrace.json"))
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--G", type=int, default=128)
    ap.add_argument("--ibeta", type=float, default=400.0)
    ap.add_argument("--eps", type=float, default=0.01)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_hashtrace.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, hashfield, hashtrace, mlp, occgrid, packed, synthetic
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
    hres = hashfield.resolutions(cfg, dev)
    grid = hashfield.update_occupancy(P, cfg, occgrid.OccupancyGrid(P["aabb"], G=a.G), prec=mlp.PREC_BF16)
    step_scale = float((P["aabb"][1] - P["aabb"][0]).max()) / 20.0
    kw = dict(eps=a.eps, step_scale=step_scale, min_step=1e-4, max_steps=128, n_bisect=8)
    with torch.no_grad():
        marched = int(packed.march(grid, o, d, nf, dt, 0, k_max=K).total)
        cap = (int(1.25 * marched) + 1023) // 1024 * 1024
        rays = packed.march(grid, o, d, nf, dt, cap, k_max=K)
        kept = int(packed.prune(rays, hashfield.density(P, cfg, rays.xyz, mlp.PREC_BF16, res=hres), early_stop_eps=1e-4, aabb=grid.aabb).total)
    prune_cap = (int(1.25 * kept) + 1023) // 1024 * 1024

    def surface():
        with torch.no_grad():
            return hashfield.render_surface(P, cfg, o, d, nf, grid=grid, prec=mlp.PREC_BF16, res=hres, **kw)

    def pruned():
        with torch.no_grad():
            return hashfield.render_packed_pruned(P, cfg, grid, o, d, nf, dt, cap, prec=mlp.PREC_BF16, k_max=K, res=hres, prune_cap=prune_cap)

    paths = {"surface": surface, "pruned": pruned}
    for fn in paths.values():  # warm-up of both shapes
        fn()
    torch.cuda.synchronize()
    rgb_s, mask_s, depth_s, _ = surface()
    rgb_p, mask_p, depth_p = pruned()[:3]
    both = (mask_s[:, 0] > 0) & (mask_p[:, 0] > 0.99)
    ln = torch.linalg.vector_norm(d, dim=-1)
    diff = ((depth_s - depth_p)[:, 0] * ln)[both]
    t = {k: [] for k in paths}
    for _ in range(5):  # alternating, so that a drifting clock hits both alike
        for name, fn in paths.items():
            t[name].append(timed(fn, reps=1)["median_ms"])
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}  # noqa: E731
    # the trace kernel alone: the library's call on buffers allocated once, on the full range and on the grid's span
    net = (P["hash.geo.0.weight"], P["hash.geo.0.bias"], P["hash.geo.2.weight"][0].contiguous(), P["hash.geo.2.bias"][:1].contiguous())
    L, _, F = P["hash.table"].shape
    t_hit, sdf_hit = torch.empty(R, device=dev), torch.empty(R, device=dev)
    status, n_eval = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    span, seen = grid.ray_span(o, d, nf)
    narrowed = torch.where(seen[:, None], span, torch.stack([nf[:, 0], torch.full_like(nf[:, 0], -math.inf)], -1)).contiguous()

    def trace(t_range):
        _lib.call("hashsdf_trace", o, d, t_range, P["aabb"], R, P["hash.table"], hres, L, cfg["log2_T"], F, *net, kw["eps"], kw["step_scale"], kw["min_step"],
                  kw["max_steps"], kw["n_bisect"], t_hit, status, n_eval, sdf_hit)

    kernels = {}
    for name, t_range in (("full t_range", nf), ("t_range narrowed by grid.ray_span", narrowed)):
        trace(t_range)
        torch.cuda.synchronize()
        ne = n_eval.view(-1, 64).float()  # a wave holds 64 consecutive rays
        live = ne.max(1).values > 0
        kernels[name] = {
            "time": timed(lambda: trace(t_range)),
            "n_eval_mean": round(float(n_eval.float().mean()), 3), "n_eval_max": int(n_eval.max()), "n_eval_total": int(n_eval.sum()),
            "n_eval_mean_over_rays_that_enter": round(float(n_eval[n_eval > 0].float().mean()), 3) if bool((n_eval > 0).any()) else 0.0,
            "status_histogram": {k: int((status == i).sum()) for i, k in enumerate(("miss", "converged", "bracketed", "starts_inside", "out_of_steps"))},
            "waves_with_work": int(live.sum()), "waves": int(ne.shape[0]),
            "lane_utilisation_sum_n_eval_over_64_max_per_wave": round(float(ne[live].sum() / (64 * ne[live].max(1).values.sum())), 4) if bool(live.any()) else None,
        }
    result = {
        "workload": "no_grad rendering of one chunk of the hash configuration: %d rays, opaque ball field (1 / beta = %g), bf16 chains, G = %d; tracer: eps = %g "
                    "(field units), step_scale = %.4g, min_step = 1e-4, max_steps = 128, n_bisect = 8; packed path: %d candidates per ray, early_stop_eps = 1e-4"
                    % (R, a.ibeta, a.G, a.eps, step_scale, K),
        "rays": R, "rays_seen_by_the_grid": int(seen.sum()), "rays_hit_by_the_tracer": int((mask_s > 0).sum()), "rays_with_packed_mask_above_0.99": int((mask_p > 0.99).sum()),
        "marched_rows": marched, "rows_after_prune": kept, "capacity": cap, "prune_capacity": prune_cap,
        "render_surface": stat(t["surface"]), "render_packed_pruned": stat(t["pruned"]),
        "ratio_of_medians_pruned_over_surface": round(statistics.median(t["pruned"]) / statistics.median(t["surface"]), 3),
        "depth_difference_metric_on_rays_both_hit": {"rays": int(both.sum()), "mean_abs": float(diff.abs().mean()) if bool(both.any()) else None,
                                                     "max_abs": float(diff.abs().max()) if bool(both.any()) else None,
                                                     "mean_signed_surface_minus_packed": float(diff.mean()) if bool(both.any()) else None},
        "rgb_max_abs_difference_on_rays_both_hit": float((rgb_s - rgb_p)[both].abs().max()) if bool(both.any()) else None,
        "trace_kernel": kernels,
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
