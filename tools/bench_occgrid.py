"""Empty-space skipping of the hash field, measured: hashfield.forward_compacted + backward on chunks of `bench.py --config hash` (1024 x 1024
frame pair, 256 samples per ray, 16 interleaved rows per chunk, bf16 chains, packed-fp16 table gradient) without a grid (the path bench.py times) and
with an occupancy grid refreshed from the field, in the same process, the two alternating; and the three occgrid kernels alone at G = 128.

Two fields: "bench" is bench.py's own (random tables, sdf_bias 0.02: density ~4 everywhere in the box, so a refreshed grid keeps every cell -- what the
grid costs when it cannot skip anything), "ball" has its density in a ball of radius 0.28 of the box (9 % of the box's volume: what skipping buys on
a scene with empty space).  Times are device-event medians of 5 repetitions after a warm-up of every shape; no number here is asserted anywhere.

    python tools/bench_occgrid.py [--out profiles/occgrid.json] [--chunks 4] [--res 1024] [--spp 256]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock_state():
    """What the driver reports (read only): clocks and power of device 0 before / after the timed work."""
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--showperflevel", "--json"], capture_output=True, text=True, timeout=10)
        card = next(iter(json.loads(r.stdout).values()))
        keep = {k: v for k, v in card.items() if re.search(r"sclk|mclk|fclk|power|performance", k, re.I)}
        return keep or {"raw": r.stdout[-400:]}
    except Exception as e:  # noqa: BLE001  (a machine without the tool still measures)
        return {"unavailable": repr(e)}


def timed(fn, reps=5):
    """median / min / max milliseconds of fn() over `reps` runs, device events around each"""
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e))
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4)}


def ball_tables(P, cfg):
    """density ~10 inside |x01 - 0.5| < 0.25, falling to ~2e-4 outside 0.3: level 0 (dense, resolution n_min) carries 20 * (0.3 - r) in feature 0,
    the geometry net passes relu(feature 0) through, sdf = 1 - relu(...)"""
    for k in ("hash.table", "hash.geo.0.weight", "hash.geo.0.bias", "hash.geo.2.weight", "hash.geo.2.bias"):
        P[k].zero_()
    n = cfg["n_min"] + 1
    ax = torch.arange(n, dtype=torch.float64) / cfg["n_min"] - 0.5
    iz, iy, ix = torch.meshgrid(ax, ax, ax, indexing="ij")
    P["hash.table"][0, :n ** 3, 0] = (20 * (0.3 - torch.sqrt(ix ** 2 + iy ** 2 + iz ** 2))).reshape(-1).float()
    P["hash.geo.0.weight"][0, 0] = 1.0
    P["hash.geo.2.weight"][0, 0] = -1.0
    P["hash.geo.2.bias"][0] = 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occgrid.json"))
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--G", type=int, default=128)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_occgrid.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, hashfield, mlp, occgrid, synthetic
    from lab4d_amd import quat_utils as Q, render_utils as RU
    _lib.lib()
    clocks = {"before": clock_state()}
    fr = synthetic.to_device(synthetic.make_frames(1, 2, a.res), dev)
    cam2field = Q.quaternion_translation_inverse(fr["field2cam"][0], fr["field2cam"][1])
    n_chunks = a.res // a.rows
    samples = []
    with torch.no_grad():
        for c in range(a.chunks):
            hxy = synthetic.make_rays(a.res, 2, rows=list(range(a.res))[c::n_chunks]).to(dev)
            out = RU.ray_samples(hxy, fr["Kinv"], fr["near_far"], cam2field, n_depth=a.spp)
            samples.append((out[4].reshape(-1, 3).contiguous(), out[5].reshape(-1, 3).contiguous()))
    S = samples[0][0].shape[0]
    result = {"workload": "forward_compacted + backward, %d chunks of 2 x %d x %d rays x %d samples (%d samples per chunk), bf16 chains, packed-fp16 table gradient"
                          % (a.chunks, a.rows, a.res, a.spp, S), "G": a.G, "fields": {}}
    for name in ("bench", "ball"):
        P, cfg = hashfield.make_weights(0, sdf_bias=0.02)
        if name == "ball":
            ball_tables(P, cfg)
        P = synthetic.to_device(P, dev)
        params = [v for k, v in P.items() if k != "aabb"]
        for v in params:
            v.requires_grad_(True)
        hres = hashfield.resolutions(cfg, dev)
        grid = occgrid.OccupancyGrid(P["aabb"], G=a.G)
        refresh = timed(lambda: hashfield.update_occupancy(P, cfg, grid, prec=mlp.PREC_BF16), reps=5)  # (the first of the five is the warm-up of its shapes)
        with torch.no_grad():
            n_box = [int(RU.compact(occgrid.OccupancyGrid(P["aabb"], G=2).mask(x))[1]) for x, _ in samples]
            n_occ = [int(RU.compact(grid.mask(x))[1]) for x, _ in samples]
        cap = {False: min(S, (int(1.25 * max(n_box)) + 1023) // 1024 * 1024), True: min(S, (int(1.25 * max(n_occ)) + 1023) // 1024 * 1024)}
        ovf = torch.zeros(1, dtype=torch.bool, device=dev)

        def run(use_grid):
            for x, d in samples:
                rgb, dens, _, o = hashfield.forward_compacted(P, cfg, x, d, cap[use_grid], prec=mlp.PREC_BF16, res=hres, table_grad_f16=True,
                                                              occ=grid if use_grid else None)
                ovf.logical_or_(o)
                (rgb.mean() + dens.mean()).backward()
            for v in params:
                v.grad = None

        for use_grid in (False, True):  # warm-up of both shapes
            run(use_grid)
        torch.cuda.synchronize()
        t = {False: [], True: []}
        for _ in range(5):  # alternating, so that a drifting clock hits both alike
            for use_grid in (False, True):
                t[use_grid].append(timed(lambda: run(use_grid), reps=1)["median_ms"])
        assert not bool(ovf), "a compaction buffer overflowed: samples were dropped"
        stat = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        result["fields"][name] = {
            "occupied_fraction": round(int(grid.n_occupied) / a.G ** 3, 4),
            "rows_after_compaction": {"box_only": n_box, "with_grid": n_occ, "capacity_box_only": cap[False], "capacity_with_grid": cap[True]},
            "without_grid": stat(t[False]), "with_grid": stat(t[True]),
            "speedup_of_medians": round(statistics.median(t[False]) / statistics.median(t[True]), 3),
            "update_occupancy": refresh}
    # the kernels alone, G = 128, on the last field's grid and the first chunk's samples / rays
    x = samples[0][0]
    R = 1 << 20
    g = torch.Generator().manual_seed(0)
    lo, ext = P["aabb"][0], P["aabb"][1] - P["aabb"][0]
    origin = (lo + (0.5 + torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)).to(dev) * ext).contiguous()
    direction = ((lo + torch.rand(R, 3, generator=g).to(dev) * ext) - origin).contiguous()
    t_range = torch.tensor([0.0, 3.0], device=dev).expand(R, 2).contiguous()
    dens = torch.rand(a.G ** 3, device=dev) * 0.02
    scratch = occgrid.OccupancyGrid(P["aabb"], G=a.G)
    for fn in (lambda: scratch.update(dens), lambda: grid.mask(x), lambda: grid.ray_span(origin, direction, t_range)):
        fn()
    torch.cuda.synchronize()
    result["kernels"] = {
        "update (G^3 = %d cells)" % a.G ** 3: timed(lambda: scratch.update(dens)),
        "mask (%d samples)" % S: timed(lambda: grid.mask(x)),
        "box test in torch, the six ops mask replaces (%d samples)" % S:
            timed(lambda: (((x - lo) / ext >= 0) & ((x - lo) / ext <= 1)).all(-1).to(torch.uint8)),
        "ray_span (%d rays through the ball grid)" % R: timed(lambda: grid.ray_span(origin, direction, t_range)),
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
