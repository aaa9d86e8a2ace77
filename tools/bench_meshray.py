"""Ray casting against a mesh, measured: lab4d_amd.meshray.MeshGrid against the marching-cubes mesh of a G^3 sphere volume (default 128^3:
54,668 faces, the mesh of tools/bench_meshsdf.py), rays of a 512^2 pinhole camera that looks at it (the corners of the image miss it).
Reported: the build time and the cast time at grid sizes 16, 32, 64, 128 and at 1 (brute force) on a reduced ray count, mean and maximum
n_tests, the divergence figure of DESIGN.md 7i (summed n_tests of a wave over 64 x the wave's maximum, on waves with work), and the SAME
first-hit algebra as chunked torch ops on the same GPU -- as in bench_meshsdf.py the only comparison there is.  Times are device-event medians
of 5 repetitions after a warm-up, the paths alternating in one process; no number here is asserted anywhere.

    python tools/bench_meshray.py [--out profiles/meshray.json] [--vol 128] [--image 512] [--brute-rays 4096]
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


def torch_first_hit(verts, faces, o, d, tr, pair_budget=1 << 23):
    """The rules of include/lab4d_meshray.h as torch ops (every face valid, no grid, no double fallback), `pair_budget` ray-face pairs at a time"""
    tri = verts[faces.long()]
    kz = d.abs().argmax(1)
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    neg = d.gather(1, kz[:, None])[:, 0] < 0
    kx, ky = torch.where(neg, ky, kx), torch.where(neg, kx, ky)
    perm = torch.stack([kx, ky, kz], 1)
    dp = d.gather(1, perm)
    S = torch.stack([dp[:, 0] / dp[:, 2], dp[:, 1] / dp[:, 2], 1 / dp[:, 2]], 1)
    t_out, f_out = [], []
    n = max(1, pair_budget // faces.shape[0])
    for s in range(0, o.shape[0], n):
        p = tri[None] - o[s:s + n, None, None]                                      # (r, F, 3 vertices, 3)
        p = p.gather(3, perm[s:s + n, None, None].expand(-1, p.shape[1], 3, -1))
        x = p[..., 0] - S[s:s + n, None, None, 0] * p[..., 2]
        y = p[..., 1] - S[s:s + n, None, None, 1] * p[..., 2]
        z = S[s:s + n, None, None, 2] * p[..., 2]
        U = x[..., 2] * y[..., 1] - y[..., 2] * x[..., 1]
        V = x[..., 0] * y[..., 2] - y[..., 0] * x[..., 2]
        W = x[..., 1] * y[..., 0] - y[..., 1] * x[..., 0]
        det = U + V + W
        t = (U * z[..., 0] + V * z[..., 1] + W * z[..., 2]) / det
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        ok = ~mixed & (det != 0) & (t >= tr[s:s + n, :1]) & (t <= tr[s:s + n, 1:])
        t = torch.where(ok, t, torch.full_like(t, float("inf")))
        best, face = t.min(1)
        t_out.append(best)
        f_out.append(torch.where(torch.isfinite(best), face, torch.full_like(face, -1)))
    return torch.cat(t_out), torch.cat(f_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshray.json"))
    ap.add_argument("--vol", type=int, default=128)
    ap.add_argument("--image", type=int, default=512)
    ap.add_argument("--brute-rays", type=int, default=4096, help="rays of the G = 1 cast and of the torch baseline (scaled up linearly)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_meshray.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, mesh, meshray
    _lib.lib()
    clocks = {"before": clock_state()}
    ax = torch.linspace(-0.5, 0.5, a.vol, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (torch.sqrt(X * X + Y * Y + Z * Z) - 0.3).contiguous()
    verts, faces = mesh.marching_cubes(vol, origin=[-0.5] * 3, step=[1.0 / (a.vol - 1)] * 3)
    F = faces.shape[0]
    # pinhole camera at (0, 0, -1.5) looking down +z; the image plane at z = 0 spans [-0.4, 0.4]^2: the sphere (r = 0.3) fills the middle
    px = (torch.arange(a.image, device=dev, dtype=torch.float32) + 0.5) / a.image * 0.8 - 0.4
    V_, U_ = torch.meshgrid(px, px, indexing="ij")
    d = torch.stack([U_, V_, torch.full_like(U_, 1.5)], -1).reshape(-1, 3).contiguous()
    o = torch.tensor([0.0, 0.0, -1.5], device=dev).expand_as(d).contiguous()
    tr = torch.stack([torch.zeros(d.shape[0], device=dev), torch.full((d.shape[0],), 2.0, device=dev)], -1).contiguous()
    R = d.shape[0]
    pick = torch.linspace(0, R - 1, a.brute_rays, device=dev).long()  # spread over the image
    ob, db, trb = o[pick].contiguous(), d[pick].contiguous(), tr[pick].contiguous()
    result = {"mesh": "marching cubes of a %d^3 sphere volume (r = 0.3 in a unit box): %d vertices, %d faces" % (a.vol, verts.shape[0], F),
              "rays": "%d^2 pinhole camera at (0, 0, -1.5), image plane [-0.4, 0.4]^2 at the sphere's centre" % a.image, "n_rays": R,
              "default_G": meshray.default_G(F),
              "comparison": "the same first-hit algebra as chunked torch ops on the same GPU, %d rays scaled up linearly (the only comparison available)" % a.brute_rays}

    sizes = (16, 32, 64, 128)
    grids = {G: meshray.MeshGrid(verts, faces, G=G) for G in sizes + (1,)}
    paths = {"build_G%d" % G: (lambda G=G: meshray.MeshGrid(verts, faces, G=G)) for G in sizes}
    paths.update({"cast_G%d" % G: (lambda G=G: grids[G].cast(o, d, tr)) for G in sizes})
    paths["cast_G1_%d_rays" % a.brute_rays] = lambda: grids[1].cast(ob, db, trb)
    paths["torch_%d_rays" % a.brute_rays] = lambda: torch_first_hit(verts, faces, ob, db, trb)
    for fn in paths.values():  # warm-up
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(5):  # the paths alternate
        for k, fn in paths.items():
            times[k].append(once(fn)[0])
    result["times"] = {k: summary(v) for k, v in times.items()}
    ref = grids[128].cast(o, d, tr)
    result["hit_fraction"] = round(float(ref.hit.float().mean()), 4)
    for G in sizes + (1,):
        h = grids[G].cast(o, d, tr) if G > 1 else grids[1].cast(ob, db, trb)
        nt = h.n_tests.float()
        waves = nt[:nt.numel() // 64 * 64].reshape(-1, 64)
        busy = waves.max(1)[0] > 0
        entry = {"list_entries": int(grids[G].cell_list.numel()), "n_tests_mean": round(float(nt.mean()), 2), "n_tests_max": int(nt.max()),
                 "waves_with_work": int(busy.sum()), "wave_sum_over_64_max": round(float((waves[busy].sum(1) / (64 * waves[busy].max(1)[0])).mean()), 3)}
        if G > 1:
            entry["equal_to_G128"] = bool(all(torch.equal(x, y) for x, y in zip(h[:5], ref[:5])))
            entry["giga_rays_per_s"] = round(R / (result["times"]["cast_G%d" % G]["median_ms"] * 1e-3) / 1e9, 3)
        result["G%d" % G] = entry
    tt, tf = torch_first_hit(verts, faces, ob, db, trb)
    mine = grids[128].cast(ob, db, trb)
    both = mine.hit & (tf >= 0)
    result["torch_vs_kernel"] = {"hit_equal": bool(torch.equal(mine.hit, tf >= 0)), "max_abs_t_diff": float((mine.t - tt)[both].abs().max()) if bool(both.any()) else 0.0}
    scale = R / a.brute_rays
    result["torch_scaled_to_all_rays_ms"] = round(result["times"]["torch_%d_rays" % a.brute_rays]["median_ms"] * scale, 2)
    result["G1_scaled_to_all_rays_ms"] = round(result["times"]["cast_G1_%d_rays" % a.brute_rays]["median_ms"] * scale, 2)
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
