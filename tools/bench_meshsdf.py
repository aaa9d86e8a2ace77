"""Signed distance from points to a mesh, measured: lab4d_amd.meshsdf.signed_distance against the marching-cubes mesh of a G^3 sphere volume
(default G = 128), for the two shapes that matter -- the G^3 cell centres of an occupancy grid (OccupancyGrid.seed_from_mesh) and 256
points (one step of NeRF.geometry_init) -- at the default slice count and at a few fixed ones.

The comparison is the SAME algebra (closest point by region classification, winding number) written as chunked torch ops on the same GPU.
pysdf, which the reference uses on the host, is not available where this project is built, so that is the only comparison there is; it is
not the reference's speed.  Throughput is point-face pairs per second, next to the fp32 vector peak of the part (256 CUs x 128 lanes x 2
flop x 2.4 GHz = 157 Tflop/s; a pair costs several hundred instructions, so the pair rate is bounded by a few hundred G pairs / s).
Times are device-event medians of 5 repetitions after a warm-up; no number here is asserted anywhere.

    python tools/bench_meshsdf.py [--out profiles/meshsdf.json] [--G 128] [--baseline-pts 4096]
"""
import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_VALU_TFLOPS = 157.3


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


def torch_signed_distance(verts, faces, pts, pair_budget=1 << 24):
    """The rules of include/lab4d_meshsdf.h as torch ops, `pair_budget` point-face pairs at a time (every face valid)."""
    tri = verts[faces.long()]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    ab, ac = b - a, c - a
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    out = []
    for o in range(0, pts.shape[0], max(1, pair_budget // faces.shape[0])):
        p = pts[o:o + max(1, pair_budget // faces.shape[0]), None, :]
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        s = va + vb + vc
        q = a + ab * (vb / s)[..., None] + ac * (vc / s)[..., None]
        for cond, cand in ((((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)), b + ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None] * (c - b)),
                           ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + (d2 / (d2 - d6))[..., None] * ac), ((d6 >= 0) & (d5 <= d6), c.expand_as(q)),
                           ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + (d1 / (d1 - d3))[..., None] * ab), ((d3 >= 0) & (d4 <= d3), b.expand_as(q)),
                           ((d1 <= 0) & (d2 <= 0), a.expand_as(q))):
            q = torch.where(cond[..., None], cand, q)
        dist2 = ((p - q) ** 2).sum(-1).min(1)[0]
        la, lb, lc = ap.norm(dim=-1), bp.norm(dim=-1), cp.norm(dim=-1)
        det = -dot(ap, torch.cross(bp, cp, dim=-1))
        den = la * lb * lc + dot(ap, bp) * lc + dot(bp, cp) * la + dot(cp, ap) * lb
        w = torch.atan2(det, den).sum(1) / (2 * math.pi)
        out.append(torch.where(w.abs() > 0.5, -1.0, 1.0) * dist2.sqrt())
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshsdf.json"))
    ap.add_argument("--G", type=int, default=128)
    ap.add_argument("--baseline-pts", type=int, default=4096, help="points of the large query the torch baseline is timed on (scaled up linearly)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_meshsdf.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, mesh, meshsdf, occgrid
    _lib.lib()
    clocks = {"before": clock_state()}
    G = a.G
    ax = torch.linspace(-0.5, 0.5, G, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sqrt(X * X + Y * Y + Z * Z) - 0.3).contiguous()
    verts, faces = mesh.marching_cubes(vol, origin=[-0.5] * 3, step=[1.0 / (G - 1)] * 3)
    F = faces.shape[0]
    aabb = torch.tensor([[-0.5] * 3, [0.5] * 3], device=dev)
    centres = occgrid.OccupancyGrid(aabb, G=G).cell_centers()
    small = (torch.rand(256, 3, generator=torch.Generator().manual_seed(0)).to(dev) - 0.5).contiguous()
    result = {"mesh": "marching cubes of a %d^3 sphere volume (r = 0.3 in a unit box): %d vertices, %d faces" % (G, verts.shape[0], F),
              "peak_fp32_valu_tflops": PEAK_FP32_VALU_TFLOPS,
              "comparison": "the same algebra as chunked torch ops on the same GPU (pysdf, the reference's host library, is not available: this is the only comparison)"}

    def pairs_per_s(n, ms):
        return round(n * F / (ms * 1e-3) / 1e9, 2)

    for name, pts, slice_counts in (("large: %d^3 cell centres" % G, centres, (None,)), ("small: 256 points", small, (None, 1, 16, 64))):
        N = pts.shape[0]
        entry = {"n_pts": N}
        for ns in slice_counts:
            n_eff = meshsdf.default_slices(N, F) if ns is None else ns
            work = torch.empty(meshsdf.work_words(N, n_eff), device=dev)
            fn = lambda: meshsdf.signed_distance(verts, faces, pts, n_slices=n_eff, work=work)  # noqa: E731
            fn()
            torch.cuda.synchronize()
            t = timed(fn)
            t.update(n_slices=n_eff, giga_pairs_per_s=pairs_per_s(N, t["median_ms"]))
            entry["default" if ns is None else "n_slices_%d" % ns] = t
        nb = min(N, a.baseline_pts)
        base_pts = pts[:nb].contiguous()
        torch_signed_distance(verts, faces, base_pts)
        torch.cuda.synchronize()
        tb = timed(lambda: torch_signed_distance(verts, faces, base_pts))
        tb.update(n_pts_timed=nb, giga_pairs_per_s=pairs_per_s(nb, tb["median_ms"]), scaled_to_n_pts_ms=round(tb["median_ms"] * N / nb, 2))
        entry["torch_baseline"] = tb
        entry["speedup_over_torch"] = round(tb["median_ms"] * N / nb / entry["default"]["median_ms"], 2)
        ours = meshsdf.signed_distance(verts, faces, base_pts)
        entry["max_abs_diff_to_torch"] = float((ours - torch_signed_distance(verts, faces, base_pts)).abs().max())
        result[name] = entry
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
