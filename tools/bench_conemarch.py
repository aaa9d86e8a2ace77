"""Cone-stepped marching through a cascade of occupancy grids, measured: the rays of one chunk of `bench.py --config hash` (2 x 16 rows x 1024
rays of a 1024 x 1024 frame pair, 32,768 rays) through a SCENE box eight times as wide as the object box, the field living on the scene box
with a ball of density inside the object box, bf16 chains, packed-fp16 table gradient.  Every ray runs from its near plane to eight times
its depth range.  Two paths, alternating in one process:
    uniform  packed.march / hashfield.render_packed on ONE G = 128 grid over the scene box at the object's step dt = (far - near) / spp
    cone     packed.march_cone / hashfield.render_packed_cone on a K = 4, G = 128 cascade (level 0 = the object box, level 3 = the scene
             box) with dt_min = that dt, dt_max = 8 dt and cone = 1 / 256
Both grids are refreshed from the field.  Reported: the kept rows of both marchers, the march alone, forward + backward of both renderers.
Times are device-event medians of 5 repetitions after a warm-up of every shape; no number here is asserted anywhere.

    python tools/bench_conemarch.py [--out profiles/conemarch.json] [--res 1024] [--spp 256] [--rows 16]
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
from bench_occgrid import clock_state, timed  # noqa: E402


def ball_tables(P, cfg, radius01):
    """tools/bench_occgrid.py's ball for a box of any size: density ~10 at the centre of the field's box, falling to ~2e-4 at `radius01` (in
    x01 units of that box) and beyond.  Level 0 (dense, resolution n_min) carries slope * (radius01 - r) in feature 0, the geometry net passes
    relu(feature 0) through, sdf = 1 - relu(...)."""
    for k in ("hash.table", "hash.geo.0.weight", "hash.geo.0.bias", "hash.geo.2.weight", "hash.geo.2.bias"):
        P[k].zero_()
    n = cfg["n_min"] + 1
    ax = torch.arange(n, dtype=torch.float64) / cfg["n_min"] - 0.5
    iz, iy, ix = torch.meshgrid(ax, ax, ax, indexing="ij")
    P["hash.table"][0, :n ** 3, 0] = (6.0 / radius01 * (radius01 - torch.sqrt(ix ** 2 + iy ** 2 + iz ** 2))).reshape(-1).float()
    P["hash.geo.0.weight"][0, 0] = 1.0
    P["hash.geo.2.weight"][0, 0] = -1.0
    P["hash.geo.2.bias"][0] = 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conemarch.json"))
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--G", type=int, default=128)
    ap.add_argument("--K", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_conemarch.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, hashfield, mlp, occgrid, packed, synthetic
    from lab4d_amd import quat_utils as Q, render_utils as RU
    _lib.lib()
    clocks = {"before": clock_state()}
    fr = synthetic.to_device(synthetic.make_frames(1, 2, a.res), dev)
    cam2field = Q.quaternion_translation_inverse(fr["field2cam"][0], fr["field2cam"][1])
    n_chunks = a.res // a.rows
    scale = 1 << (a.K - 1)
    with torch.no_grad():
        hxy = synthetic.make_rays(a.res, 2, rows=list(range(a.res))[0::n_chunks]).to(dev)
        out = RU.ray_samples(hxy, fr["Kinv"], fr["near_far"], cam2field, n_depth=2)  # two depths per ray: the ray's origin and direction in the field's frame
        x, depth = out[4].reshape(-1, 2, 3), out[3].reshape(-1, 2, 1)
        d = ((x[:, 1] - x[:, 0]) / (depth[:, 1] - depth[:, 0])).contiguous()  # per unit of depth
        o = (x[:, 0] - depth[:, 0] * d).contiguous()
        R = o.shape[0]
        nf = fr["near_far"][:, None, :].expand(2, R // 2, 2).reshape(R, 2).contiguous()
        span = nf[:, 1] - nf[:, 0]
        tr = torch.stack([nf[:, 0], nf[:, 0] + scale * span], 1).contiguous()  # from the near plane through `scale` depth ranges
    dt = float(span.max()) / a.spp
    k_uniform = scale * a.spp
    cone, dt_max, k_cone = 1.0 / 256.0, scale * dt, scale * a.spp
    P, cfg = hashfield.make_weights(0, sdf_bias=0.02)
    obj = P["aabb"].to(dev)
    casc = occgrid.OccupancyCascade(obj, K=a.K, G=a.G)
    P["aabb"] = casc.aabbs[a.K - 1].view(2, 3).cpu().clone()  # the field lives on the scene box
    ball_tables(P, cfg, 0.3 / scale)
    P = synthetic.to_device(P, dev)
    params = [v for k, v in P.items() if k != "aabb"]
    for v in params:
        v.requires_grad_(True)
    hres = hashfield.resolutions(cfg, dev)
    grid = hashfield.update_occupancy(P, cfg, occgrid.OccupancyGrid(P["aabb"], G=a.G), prec=mlp.PREC_BF16)
    hashfield.update_occupancy_cascade(P, cfg, casc, prec=mlp.PREC_BF16, chunk=1 << 21)
    with torch.no_grad():
        kept_u = int(packed.march(grid, o, d, tr, dt, 0, k_max=k_uniform).total)
        kept_c = int(packed.march_cone(casc, o, d, tr, cone, dt, dt_max, 0, k_max=k_cone).total)
    cap_u, cap_c = ((int(1.25 * n) + 1023) // 1024 * 1024 for n in (kept_u, kept_c))
    ovf = torch.zeros(1, dtype=torch.bool, device=dev)

    def finish(res, backward):
        rgb, mask, depth_r, _, ov = res
        ovf.logical_or_(ov)
        if backward:
            (rgb.mean() + mask.mean() + depth_r.mean()).backward()
            for v in params:
                v.grad = None
        return rgb, mask, depth_r

    def uniform(backward=True):
        return finish(hashfield.render_packed(P, cfg, grid, o, d, tr, dt, cap_u, prec=mlp.PREC_BF16, table_grad_f16=True, k_max=k_uniform, res=hres), backward)

    def cone_path(backward=True):
        return finish(hashfield.render_packed_cone(P, cfg, casc, o, d, tr, cone, dt, dt_max, cap_c, prec=mlp.PREC_BF16, table_grad_f16=True, k_max=k_cone,
                                                   res=hres), backward)

    def march_u():
        return packed.march(grid, o, d, tr, dt, cap_u, k_max=k_uniform)

    def march_c():
        return packed.march_cone(casc, o, d, tr, cone, dt, dt_max, cap_c, k_max=k_cone)

    paths = {"render_packed (uniform)": uniform, "render_packed_cone": cone_path, "march (uniform)": march_u, "march_cone": march_c}
    for fn in paths.values():  # warm-up of every shape
        fn()
    torch.cuda.synchronize()
    with torch.no_grad():
        a_, b_ = uniform(False), cone_path(False)
        differ = {k: float((x - y).abs().max()) for k, x, y in zip(("rgb", "mask", "depth"), b_, a_)}  # (two samplings of one field: not an error figure)
        levels = torch.bincount(march_c().level.long() + 1, minlength=a.K + 1)[1:].tolist()
    t = {k: [] for k in paths}
    for _ in range(5):  # alternating, so that a drifting clock hits both alike
        for name, fn in paths.items():
            t[name].append(timed(fn, reps=1)["median_ms"])
    assert not bool(ovf), "a packed buffer overflowed: samples were dropped"
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    med = lambda k: statistics.median(t[k])
    result = {
        "workload": "one chunk of the hash configuration: %d rays from the near plane through %d depth ranges, a scene box %d times the object box, a "
                    "ball of density in the object box, bf16 chains, packed-fp16 table gradient, G = %d" % (R, scale, scale, a.G),
        "dt": dt, "uniform": {"k_max": k_uniform, "kept_rows": kept_u, "capacity": cap_u, "occupied_fraction": round(int(grid.n_occupied) / a.G ** 3, 5)},
        "cone": {"K": a.K, "cone": cone, "dt_min": dt, "dt_max": dt_max, "k_max": k_cone, "kept_rows": kept_c, "capacity": cap_c, "rows_per_level": levels,
                 "occupied_fraction_per_level": [round(n / a.G ** 3, 5) for n in casc.n_occupied.tolist()]},
        "march_ms": {"uniform: count + scan + write": stat(t["march (uniform)"]), "cone: count + scan + write": stat(t["march_cone"])},
        "forward_backward_ms": {"render_packed on the single scene grid": stat(t["render_packed (uniform)"]), "render_packed_cone": stat(t["render_packed_cone"])},
        "ratio_of_medians": {"kept_rows uniform / cone": round(kept_u / max(kept_c, 1), 3), "march uniform / cone": round(med("march (uniform)") / med("march_cone"), 3),
                             "forward + backward uniform / cone": round(med("render_packed (uniform)") / med("render_packed_cone"), 3)},
        "max_abs_difference_of_the_two_renderings": differ,
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
