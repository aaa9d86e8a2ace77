"""The hash field's fused SDF gradient, measured (csrc/hashsdf.hip through hashfield.sdf_gradient / eikonal_loss), at the default hash
configuration (L 16, F 2, T 2^19, n_max 2048) and two sizes:
    eikonal  the eikonal subset of one chunk of `bench.py --config hash`: 1/16 of its 2 x 16 x 1024 rays x 256 samples = 524,288 points,
             uniform in the box, table of hashfield.make_weights x 1e3
    packed   the kept rows of tools/bench_packed.py's ball field (its rays, its grid, its march; 82,063 rows at the defaults)
For each: the forward alone (sdf + gradient, no_grad) and forward + backward of eikonal_loss(...).mean() to the table and the geometry
net.  Next to them the only first-order alternative that exists without this kernel: autograd.grad(forward(get_density=False).sum(), xyz)
at PREC_F32 (encoding forward, both chains forward, both chains backward, encoding backward to the point) -- it gives the gradient but
nothing can be differentiated through it.  Times are device-event medians of 5 repetitions after a warm-up; no ratio is asserted anywhere:
the capability has no predecessor.

    python tools/bench_hashsdf.py [--out profiles/hashsdf.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_occgrid import ball_tables, clock_state, timed  # noqa: E402


def packed_rows(dev, res=1024, spp=256, rows=16, G=128):
    """the kept rows of tools/bench_packed.py (the same rays, field, grid and march) and the field they belong to"""
    from lab4d_amd import hashfield, mlp, occgrid, packed, synthetic
    from lab4d_amd import quat_utils as Q, render_utils as RU
    fr = synthetic.to_device(synthetic.make_frames(1, 2, res), dev)
    cam2field = Q.quaternion_translation_inverse(fr["field2cam"][0], fr["field2cam"][1])
    with torch.no_grad():
        hxy = synthetic.make_rays(res, 2, rows=list(range(res))[0::res // rows]).to(dev)
        out = RU.ray_samples(hxy, fr["Kinv"], fr["near_far"], cam2field, n_depth=2)
        x, depth = out[4].reshape(-1, 2, 3), out[3].reshape(-1, 2, 1)
        d = ((x[:, 1] - x[:, 0]) / (depth[:, 1] - depth[:, 0])).contiguous()
        o = (x[:, 0] - depth[:, 0] * d).contiguous()
        R = o.shape[0]
        nf = fr["near_far"][:, None, :].expand(2, R // 2, 2).reshape(R, 2).contiguous()
    dt = float((nf[:, 1] - nf[:, 0]).max()) / spp
    P, cfg = hashfield.make_weights(0, sdf_bias=0.02)
    ball_tables(P, cfg)
    P = synthetic.to_device(P, dev)
    grid = hashfield.update_occupancy(P, cfg, occgrid.OccupancyGrid(P["aabb"], G=G), prec=mlp.PREC_BF16)
    with torch.no_grad():
        kept = int(packed.march(grid, o, d, nf, dt, 0, k_max=spp).total)
        rays = packed.march(grid, o, d, nf, dt, kept, k_max=spp)
    return P, cfg, rays.xyz[:kept].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hashsdf.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_hashsdf.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, hashfield, mlp, synthetic
    _lib.lib()
    clocks = {"before": clock_state()}
    cases = {}
    P, cfg = hashfield.make_weights(0)
    P["hash.table"] *= 1e3
    P = synthetic.to_device(P, dev)
    S = 2 * 16 * 1024 * 256 // 16
    g = torch.Generator(device=dev).manual_seed(1)
    lo, hi = P["aabb"][0], P["aabb"][1]
    cases["eikonal"] = (P, cfg, (lo + torch.rand(S, 3, device=dev, generator=g) * (hi - lo)).contiguous())
    cases["packed"] = packed_rows(dev)
    results = {}
    for name, (P, cfg, xyz) in cases.items():
        names = ["hash.table", "hash.geo.0.weight", "hash.geo.0.bias", "hash.geo.2.weight", "hash.geo.2.bias"]
        for k in names:
            P[k].requires_grad_(True)
        hres = hashfield.resolutions(cfg, dev)
        n = xyz.shape[0]
        dirs = torch.zeros_like(xyz)
        dirs[:, 2] = 1.0

        def fwd():
            with torch.no_grad():
                return hashfield.sdf_gradient(P, cfg, xyz, res=hres)

        def fwd_bwd():
            return torch.autograd.grad(hashfield.eikonal_loss(P, cfg, xyz, res=hres).mean(), [P[k] for k in names], allow_unused=True)

        def first_order():
            xr = xyz.clone().requires_grad_(True)
            sdf = hashfield.forward(P, cfg, xr, dirs, spf=n, prec=mlp.PREC_F32, res=hres, get_density=False)[1]
            return torch.autograd.grad(sdf.sum(), xr)

        for fn in (fwd, fwd_bwd, first_order):
            fn()
        torch.cuda.synchronize()
        results[name] = {"points": n, "inside_share": round(float((((xyz - P["aabb"][0]) / (P["aabb"][1] - P["aabb"][0]) >= 0).all(-1)
                                                                   & ((xyz - P["aabb"][0]) / (P["aabb"][1] - P["aabb"][0]) <= 1).all(-1)).float().mean()), 4),
                         "fused_forward": timed(fwd), "fused_forward_backward_eikonal": timed(fwd_bwd),
                         "first_order_alternative_f32": timed(first_order)}
        print(name, json.dumps(results[name]))
    clocks["after"] = clock_state()
    doc = {"tool": "tools/bench_hashsdf.py", "config": cases["eikonal"][1], "timing": "device events, median / min / max of 5 after a warm-up",
           "note": "no ratio is asserted: the capability has no predecessor; the first-order alternative yields the gradient only, nothing differentiable",
           "results": results, "clocks": clocks}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
