"""Packed ray marching of the hash field, measured: one chunk of `bench.py --config hash` (2 x 16 rows x 1024 rays of a 1024 x 1024 frame pair)
with the ball-shaped field of tools/bench_occgrid.py (density in a ball of 9 % of the box), bf16 chains, packed-fp16 table gradient, a G = 128
occupancy grid refreshed from the field.  Two paths over the SAME candidate lattice t_k = near + (k + 0.5) dt, k < spp, alternating in one
process:
    dense   the path before packed marching: all spp candidates of every ray as (S, 3) points and directions, forward_compacted(occ=grid),
            scatter into (S, .), render_utils.compute_weights + the normalised sums over R x spp entries
    packed  hashfield.render_packed: packed.march, the field on the packed rows, packed.composite
Forward + backward of each, the march and the two composite kernels alone (the library's calls, without autograd or torch glue), the kept-sample count and the peak memory of both paths.  Times are
device-event medians of 5 repetitions after a warm-up of every shape; no number here is asserted anywhere.

    python tools/bench_packed.py [--out profiles/packed.json] [--res 1024] [--spp 256] [--rows 16]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed.json"))
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--G", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_packed.py measures on the GPU; none found (there is no CPU path)")
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
    params = [v for k, v in P.items() if k != "aabb"]
    for v in params:
        v.requires_grad_(True)
    hres = hashfield.resolutions(cfg, dev)
    grid = hashfield.update_occupancy(P, cfg, occgrid.OccupancyGrid(P["aabb"], G=a.G), prec=mlp.PREC_BF16)
    with torch.no_grad():
        kept = int(packed.march(grid, o, d, nf, dt, 0, k_max=K).total)
    cap = (int(1.25 * kept) + 1023) // 1024 * 1024
    S = R * K
    ovf = torch.zeros(1, dtype=torch.bool, device=dev)

    def dense(backward=True):
        with torch.no_grad():
            tk = nf[:, :1] + (torch.arange(K, device=dev, dtype=torch.float32) + 0.5)[None, :] * dt
            xyz = (o[:, None, :] + tk[:, :, None] * d[:, None, :]).reshape(S, 3)
            ln = d.norm(dim=-1, keepdim=True)
            dirs = (d / ln)[:, None, :].expand(R, K, 3).reshape(S, 3).contiguous()
            deltas = (dt * ln).expand(R, K).contiguous()
        rgb_s, dens_s, _, ov = hashfield.forward_compacted(P, cfg, xyz, dirs, cap, prec=mlp.PREC_BF16, res=hres, table_grad_f16=True, occ=grid)
        ovf.logical_or_(ov)
        w, _ = RU.compute_weights(dens_s.reshape(1, R, K, 1), deltas.reshape(1, R, K, 1))
        w = w.reshape(R, K)
        mask = w.sum(-1, keepdim=True)
        wn = w / (mask + 1e-6)
        rgb = (wn[:, :, None] * rgb_s.reshape(R, K, 3)).sum(1)
        depth_r = (wn * tk).sum(1, keepdim=True)
        if backward:
            (rgb.mean() + mask.mean() + depth_r.mean()).backward()
            for v in params:
                v.grad = None
        return rgb, mask, depth_r

    def packed_path(backward=True):
        rgb, mask, depth_r, _, ov = hashfield.render_packed(P, cfg, grid, o, d, nf, dt, cap, prec=mlp.PREC_BF16, table_grad_f16=True, k_max=K, res=hres)
        ovf.logical_or_(ov)
        if backward:
            (rgb.mean() + mask.mean() + depth_r.mean()).backward()
            for v in params:
                v.grad = None
        return rgb, mask, depth_r

    paths = {"dense": dense, "packed": packed_path}
    peak = {}
    for name, fn in paths.items():  # warm-up of both shapes, and the peak memory of one forward + backward
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    with torch.no_grad():
        a_, b_ = dense(False), packed_path(False)
        agree = {k: float((x - y).abs().max()) for k, x, y in zip(("rgb", "mask", "depth"), b_, a_)}
    t = {k: [] for k in paths}
    for _ in range(5):  # alternating, so that a drifting clock hits both alike
        for name, fn in paths.items():
            t[name].append(timed(fn, reps=1)["median_ms"])
    assert not bool(ovf), "a packed buffer overflowed: samples were dropped"
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    # the kernels alone: march through its Python entry (two launches around torch.cumsum, and its allocations), the compositing pair as
    # the library's two calls on buffers allocated once (no autograd, no reductions, no fills)
    with torch.no_grad():
        rays = packed.march(grid, o, d, nf, dt, cap, k_max=K)
        dens = torch.rand(cap, device=dev) * 10
        rgb_s = torch.rand(cap, 3, device=dev)
        depth_s = rays.t[:, None].contiguous()
    fl, sumC = packed._field_list([rgb_s, depth_s], [0, 0])
    c_mask, c_out = torch.empty(R, device=dev), torch.empty(R, sumC, device=dev)
    g_mask, g_out = torch.ones(R, device=dev), torch.ones(R, sumC, device=dev)
    g_dens, g_rgb = torch.zeros(cap, device=dev), torch.zeros(cap, 3, device=dev)
    gf = _lib.FieldGrads()
    gf.n_fields = 2
    gf.fields[0], gf.fields[1] = _lib.dp(g_rgb), None  # (the gradients render_packed asks for: density and colour)

    def comp_fwd():
        _lib.call("packed_composite_forward", dens, rays.deltas, fl, rays.ray_start, rays.ray_count, R, cap, None, None, c_mask, c_out)

    def comp_bwd():
        _lib.call("packed_composite_backward", dens, rays.deltas, fl, rays.ray_start, rays.ray_count, R, cap, g_mask, g_out, g_dens, None, gf)

    result = {
        "workload": "forward + backward of one chunk of the hash configuration: %d rays x %d candidates (%d lattice points), ball field, bf16 chains, "
                    "packed-fp16 table gradient, G = %d" % (R, K, S, a.G),
        "dt": dt, "kept_samples": kept, "kept_fraction": round(kept / S, 4), "capacity": cap,
        "occupied_fraction": round(int(grid.n_occupied) / a.G ** 3, 4),
        "dense_lattice_through_forward_compacted": stat(t["dense"]), "render_packed": stat(t["packed"]),
        "speedup_of_medians": round(statistics.median(t["dense"]) / statistics.median(t["packed"]), 3),
        "peak_memory_MiB": peak, "max_abs_difference_packed_vs_dense": agree,
        "kernels": {
            "march: count + scan + write (%d rays -> %d rows)" % (R, kept): timed(lambda: packed.march(grid, o, d, nf, dt, cap, k_max=K)),
            "composite forward kernel (%d rows, rgb + depth)" % cap: timed(comp_fwd),
            "composite backward kernel (gradients of density and rgb)": timed(comp_bwd),
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
