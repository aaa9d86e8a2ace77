"""Camera-visibility culling of a cascade of occupancy grids, measured: the scene of tools/bench_conemarch.py (a K = 4, G = 128 cascade whose
level 0 is the object box and whose level 3, the scene box, is eight times as wide; the field lives on the scene box: a ball of density in
the object box plus noise in the table, which stands for the entries no ray ever trained) and M = 512 views on a ring around the object box,
looking at its centre.  Reported:
    mark     lab4d_occvis_mark (all K levels, one launch) at min_views = 1, and at min_views = M, where no wave can leave the loop over the
             views early: the work bound K G^3 M 6 plane tests, executed
    torch    the same rule as chunked torch ops on the device (fp32, no early exit): the comparator, not the code under test; its marks are
             compared with the kernel's, and the number of views each wave of 64 cells has to test before all of them have min_views is
             counted from it
    cull     n_occupied per level before and after cascade.cull_invisible
    refresh  hashfield.update_occupancy_cascade on the culled cascade, full and with visible_only=True at a capacity of the refresh set
Times are device-event medians of 5 repetitions after a warm-up; no number here is asserted anywhere.

    python tools/bench_occgrid_cull.py [--out profiles/occvis_bench.json] [--G 128] [--K 4] [--M 512]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_conemarch import ball_tables  # noqa: E402
from bench_occgrid import clock_state, timed  # noqa: E402


def ring_cameras(M, centre, radius, res, dev):
    """Kmat (M, 4), field2cam (M, 4, 4) float64: M cameras on a circle around `centre`, a quarter of the radius above its plane, +z at the centre"""
    a = 2 * math.pi * torch.arange(M, dtype=torch.float64) / M
    eye = centre + radius * torch.stack([torch.cos(a), torch.sin(a), torch.full_like(a, 0.25)], 1)
    z = torch.nn.functional.normalize(centre - eye, dim=1)
    x = torch.nn.functional.normalize(torch.linalg.cross(z, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(z)), dim=1)
    y = torch.linalg.cross(z, x)
    E = torch.eye(4, dtype=torch.float64).repeat(M, 1, 1)
    E[:, :3, :3] = torch.stack([x, y, z], 1)
    E[:, :3, 3] = -torch.einsum("mij,mj->mi", E[:, :3, :3], eye)
    Kmat = torch.tensor([1.2 * res, 1.2 * res, res / 2, res / 2], dtype=torch.float64).repeat(M, 1)
    return Kmat.to(dev), E.to(dev)


@torch.no_grad()
def torch_mark(planes, casc, min_views, cells=1 << 16, views=64):
    """The rule of include/lab4d_occvis.h in fp32 torch ops, chunked: (visible (K, G^3) bool, first (K, G^3) int32 = the number of views a
    cell needs before it has min_views, M where it never does)"""
    K, G, M = casc.K, casc.G, planes.shape[0]
    n, ab, d = planes[:, :, :3], planes[:, :, :3].abs(), planes[:, :, 3]
    ok = torch.isfinite(planes).all(-1).all(-1)
    ctr = casc.cell_centers()
    out_v, out_f = [], []
    for lv in range(K):
        h = (casc.aabbs[lv, 3:] - casc.aabbs[lv, :3]) / (2 * G)
        vis, first = [], []
        for o in range(0, G ** 3, cells):
            c = ctr[lv, o:o + cells]
            q = c.abs() + h
            seen = torch.zeros(c.shape[0], dtype=torch.int32, device=c.device)
            need = torch.full((c.shape[0],), M, dtype=torch.int32, device=c.device)
            for m in range(0, M, views):
                v = torch.einsum("ca,mpa->cmp", c, n[m:m + views]) + (ab[m:m + views] @ h) + d[m:m + views]
                slack = 2.0 ** -19 * (torch.einsum("ca,mpa->cmp", q, ab[m:m + views]) + d[m:m + views].abs())
                s = ((v >= -slack).all(-1) & ok[m:m + views]).to(torch.int32)
                run = seen[:, None] + s.cumsum(1)
                hit = run >= min_views
                at = torch.where(hit.any(1), m + 1 + hit.to(torch.int32).argmax(1).to(torch.int32), torch.full_like(need, M))
                need = torch.minimum(need, at)
                seen = run[:, -1].contiguous()
            vis.append(seen >= min_views)
            first.append(need)
        out_v.append(torch.cat(vis))
        out_f.append(torch.cat(first))
    return torch.stack(out_v), torch.stack(out_f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occvis_bench.json"))
    ap.add_argument("--G", type=int, default=128)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--res", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_occgrid_cull.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, hashfield, mlp, occgrid, synthetic
    _lib.lib()
    clocks = {"before": clock_state()}
    K, G, M = a.K, a.G, a.M
    scale = 1 << (K - 1)
    P, cfg = hashfield.make_weights(0, sdf_bias=0.02)
    obj = P["aabb"].to(dev)
    casc = occgrid.OccupancyCascade(obj, K=K, G=G)
    P["aabb"] = casc.aabbs[K - 1].view(2, 3).cpu().clone()  # the field lives on the scene box
    ball_tables(P, cfg, 0.3 / scale)
    n0 = (cfg["n_min"] + 1) ** 3
    P["hash.table"][0, :n0, 0] += 0.5 * torch.randn(n0, generator=torch.Generator().manual_seed(1))  # untrained entries: noise around the threshold
    P = synthetic.to_device(P, dev)
    centre = (obj[0] + obj[1]).double().cpu() / 2
    radius = 3.0 * float(torch.linalg.vector_norm((obj[1] - obj[0]).double() / 2))
    Kmat, E = ring_cameras(M, centre, radius, a.res, dev)
    planes = occgrid.camera_planes(Kmat, E, (a.res, a.res), near=0.05 * radius)

    def mark(mv):
        return occgrid._mark_visible(planes, casc.aabbs, K, G, mv)

    mark(1), mark(M)
    torch.cuda.synchronize()
    t_mark, t_full = timed(lambda: mark(1)), timed(lambda: mark(M))
    vis_words, n_vis = mark(1)
    ref_vis, first = torch_mark(planes, casc, 1)
    t_torch = timed(lambda: torch_mark(planes, casc, 1), reps=2)
    kernel_vis = occgrid.unpack_bits(vis_words, G)
    per_wave = torch.nn.functional.pad(first, (0, -G ** 3 % 64), value=0).reshape(K, -1, 64).amax(-1)  # views a wave tests before all its cells are seen
    bound = K * G ** 3 * M * 6
    hashfield.update_occupancy_cascade(P, cfg, casc, prec=mlp.PREC_BF16, chunk=1 << 21)
    before = casc.n_occupied.tolist()
    casc.cull_invisible(planes)
    after = casc.n_occupied.tolist()
    need = int(casc.refresh_set().sum())
    cap = (need + 1023) // 1024 * 1024
    ovf = torch.zeros(1, dtype=torch.bool, device=dev)

    def full():
        hashfield.update_occupancy_cascade(P, cfg, casc, prec=mlp.PREC_BF16, chunk=1 << 21)

    def lean():
        ovf.logical_or_(hashfield.update_occupancy_cascade(P, cfg, casc, prec=mlp.PREC_BF16, chunk=1 << 21, visible_only=True, cap=cap)[1])

    full(), lean()
    torch.cuda.synchronize()
    t_ref = {"full": [], "visible_only": []}
    for _ in range(5):  # alternating, so that a drifting clock hits both alike
        t_ref["full"].append(timed(full, reps=1)["median_ms"])
        t_ref["visible_only"].append(timed(lean, reps=1)["median_ms"])
    assert not bool(ovf), "the refresh buffer overflowed"
    stat = lambda v: {"median_ms": round(sorted(v)[len(v) // 2], 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    result = {
        "workload": "K = %d, G = %d cascade, scene box %d times the object box, M = %d views on a ring of radius %.3g around the object box, %d x %d pixels, "
                    "focal 1.2 x the width, no far plane" % (K, G, scale, M, radius, a.res, a.res),
        "mark_ms": {"occvis_mark, min_views = 1": t_mark, "occvis_mark, min_views = M (no early exit: the whole work bound)": t_full,
                    "the same rule as chunked torch ops (comparator)": t_torch},
        "plane_tests": {"work bound K G^3 M 6": bound, "executed at min_views = 1 (64 lanes x the views each wave tests x 6)": int(per_wave.sum()) * 64 * 6,
                        "share of the bound": round(int(per_wave.sum()) * 64 * 6 / bound, 4),
                        "time at min_views = 1 over time at min_views = M": round(t_mark["median_ms"] / t_full["median_ms"], 4)},
        "cells_where_kernel_and_torch_comparator_differ": int((kernel_vis != ref_vis).sum()),
        "n_visible_per_level": n_vis.tolist(), "n_visible_after_raising_to_the_parents": casc.n_visible.tolist(),
        "n_occupied_per_level": {"before": before, "after": after},
        "refresh_ms": {"update_occupancy_cascade, full (K G^3 = %d points)" % (K * G ** 3): stat(t_ref["full"]),
                       "update_occupancy_cascade, visible_only (refresh set %d points, capacity %d)" % (need, cap): stat(t_ref["visible_only"])},
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
