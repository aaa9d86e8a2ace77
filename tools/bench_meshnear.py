"""Closest point and signed distance through the face grid, measured: lab4d_amd.meshray.MeshGrid.closest against the brute-force
lab4d_amd.meshsdf.signed_distance (csrc/meshsdf.hip, which this feature leaves as it was) on the marching-cubes mesh of a G^3 sphere volume
(default 128^3: 54,668 faces, the mesh of tools/bench_meshsdf.py).  Three query shapes: the cell centres of a 128^3 lattice over the grid's
default box, the same lattice over a box twice the mesh's extent, and 256 points (geometry_init's batch).  Reported per grid size 16 / 32 / 64 /
128: the signed and the unsigned time, mean and maximum n_tests, the divergence figure of DESIGN.md 7j (summed n_tests of a wave over 64 x the
wave's maximum), the cells a point visits (from the CPU twin on a sample: the kernel does not count them), equality with brute force, and the
honest worst case: points far outside the box, which walk every cell and every list entry.  Times are device-event medians of 5 repetitions
after a warm-up, the paths alternating in one process; no number here is asserted anywhere.

    python tools/bench_meshnear.py [--out profiles/meshnear.json] [--vol 128] [--lattice 128] [--coarse 32] [--sample 1024]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_meshsdf import clock_state  # noqa: E402


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def lattice(box, n):
    ax = (torch.arange(n, device=box.device, dtype=torch.float32) + 0.5) / n
    return (box[0] + torch.cartesian_prod(ax, ax, ax) * (box[1] - box[0])).contiguous()


def twin_cells(verts, faces, G, box, pts):
    """cells visited per point, from the CPU twin (the kernel keeps no such count)"""
    import meshnear_checks as NC
    import meshray_checks as MC
    grid = MC.host_build(MC.build_host(), verts.cpu().numpy(), faces.cpu().numpy(), G, aabb=box.cpu().numpy())
    return NC.host_closest(NC.build_host(), grid, pts.cpu().numpy(), 0, 1)["n_cells"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshnear.json"))
    ap.add_argument("--vol", type=int, default=128)
    ap.add_argument("--lattice", type=int, default=128)
    ap.add_argument("--coarse", type=int, default=32, help="lattice of the double box at G >= 64 (scaled up to --lattice)")
    ap.add_argument("--sample", type=int, default=1024, help="points of the far set and of the CPU twin's cell count")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_meshnear.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, mesh, meshray, meshsdf
    _lib.lib()
    clocks = {"before": clock_state()}
    ax = torch.linspace(-0.5, 0.5, a.vol, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sqrt(X * X + Y * Y + Z * Z) - 0.3).contiguous()
    verts, faces = mesh.marching_cubes(vol, origin=[-0.5] * 3, step=[1.0 / (a.vol - 1)] * 3)
    F = faces.shape[0]
    box = meshray.default_aabb(verts)
    mid, half = (box[0] + box[1]) / 2, (box[1] - box[0]) / 2
    wide = torch.stack([mid - 2 * half, mid + 2 * half])
    g = torch.Generator(device="cpu").manual_seed(0)
    shapes = {"lattice_default_box": lattice(box, a.lattice), "lattice_double_box": lattice(wide, a.lattice),
              "256_points": (mid + (torch.rand(256, 3, generator=g).to(dev) * 2 - 1) * 1.5 * half).contiguous()}
    dirs = torch.nn.functional.normalize(torch.randn(a.sample, 3, generator=g), dim=-1).to(dev)
    far = (mid + dirs * 8 * 2 * half.max()).contiguous()
    result = {"mesh": "marching cubes of a %d^3 sphere volume (r = 0.3 in a unit box): %d vertices, %d faces" % (a.vol, verts.shape[0], F),
              "shapes": {k: int(v.shape[0]) for k, v in shapes.items()}, "default_G": meshray.default_G(F),
              "comparison": "lab4d_amd.meshsdf.signed_distance (brute force, csrc/meshsdf.hip as before this feature) in the same process"}
    sizes = (16, 32, 64, 128)
    grids = {G: meshray.MeshGrid(verts, faces, G=G) for G in sizes}
    for G in sizes:
        grids[G].orientation()
    # Outside the box a point walks (nearly) every cell and every list entry -- more than brute force --, so the double box at G >= 64 is timed on
    # a coarser lattice over the same box and scaled up linearly (as tools/bench_meshray.py scales its G = 1 cast); the JSON says where.
    coarse = lattice(wide, a.coarse)
    scaled = {(G, "lattice_double_box"): shapes["lattice_double_box"].shape[0] / coarse.shape[0] for G in sizes if G >= 64}
    paths = {}
    for name, pts in shapes.items():
        paths["brute/%s" % name] = lambda pts=pts: meshsdf.signed_distance(verts, faces, pts)
        for G in sizes:
            if (G, name) in scaled:
                pts = coarse
            paths["G%d/signed/%s" % (G, name)] = lambda G=G, pts=pts: grids[G].closest(pts)
            paths["G%d/unsigned/%s" % (G, name)] = lambda G=G, pts=pts: grids[G].closest(pts, sign=None)
    paths["brute/far_%d" % a.sample] = lambda: meshsdf.signed_distance(verts, faces, far)
    for G in sizes:
        paths["G%d/signed/far_%d" % (G, a.sample)] = lambda G=G: grids[G].closest(far)
    for k, fn in paths.items():  # warm-up
        print("[bench_meshnear] warm-up %s: %.1f ms" % (k, once(fn)[0]), file=sys.stderr, flush=True)
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for rep in range(5):  # the paths alternate
        for k, fn in paths.items():
            times[k].append(once(fn)[0])
        print("[bench_meshnear] repetition %d done" % rep, file=sys.stderr, flush=True)
    result["times"] = {k: summary(v) for k, v in times.items()}
    for (G, name), factor in scaled.items():
        for kind in ("signed", "unsigned"):
            t = result["times"]["G%d/%s/%s" % (G, kind, name)]
            t["timed_points"], t["scaled_to_all_points_ms"] = int(coarse.shape[0]), round(t["median_ms"] * factor, 2)
    shapes["far_%d" % a.sample] = far
    for name, pts in shapes.items():
        sdf_b, face_b, q_b = meshsdf.signed_distance(verts, faces, pts, return_face=True, return_closest=True)
        pick = torch.linspace(0, pts.shape[0] - 1, min(a.sample, pts.shape[0]), device=dev).long()
        for G in sizes:
            if (G, name) in scaled:  # the figures of the coarser lattice, which the times are of
                pts = coarse
                sdf_b, face_b, q_b = meshsdf.signed_distance(verts, faces, pts, return_face=True, return_closest=True)
                pick = torch.linspace(0, pts.shape[0] - 1, min(a.sample, pts.shape[0]), device=dev).long()
            print("[bench_meshnear] figures of %s at G = %d" % (name, G), file=sys.stderr, flush=True)
            near = grids[G].closest(pts)
            nt = near.n_tests.float()
            waves = nt[:nt.numel() // 64 * 64].reshape(-1, 64)
            # (a far point is farther from every face than from any plane of the grid: its walk never stops early and visits all G^3 cells)
            is_far = name.startswith("far")
            cells = None if is_far else twin_cells(verts, faces, G, box, pts[pick])
            off = sdf_b.abs() > 1e-5 * float(torch.linalg.vector_norm(box[1] - box[0]))
            result.setdefault("G%d" % G, {"list_entries": int(grids[G].cell_list.numel())})[name] = {
                "n_tests_mean": round(float(nt.mean()), 2), "n_tests_max": int(nt.max()),
                "wave_sum_over_64_max": round(float((waves.sum(1) / (64 * waves.max(1)[0].clamp(min=1))).mean()), 3),
                **({"cells_visited_derived_not_counted": G ** 3} if is_far else
                   {"cells_visited_mean": round(float(cells.mean()), 1), "cells_visited_max": int(cells.max())}),
                "d_face_closest_equal_to_brute": bool(torch.equal(near.sdf.abs(), sdf_b.abs()) and torch.equal(near.face, face_b) and torch.equal(near.closest, q_b)),
                "sign_equal_off_surface": bool(torch.equal(near.sdf[off] < 0, sdf_b[off] < 0)),
                "points": int(pts.shape[0]),
                "speedup_signed": round(result["times"]["brute/%s" % name]["median_ms"] / result["times"]["G%d/signed/%s" % (G, name)].get(
                    "scaled_to_all_points_ms", result["times"]["G%d/signed/%s" % (G, name)]["median_ms"]), 3)}
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
