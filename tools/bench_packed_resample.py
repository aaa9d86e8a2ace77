"""Importance resampling of a packed sample list per ray (include/lab4d_presample.h), measured.
  timing   R rays with about n rows per ray (counts uniform in [n / 2, 3 n / 2], no gaps, unit directions, a random density with a peak
           somewhere along every ray), for every n of --rows, n_imp = --n-imp new rows per ray:
    kernels  the library's calls alone on buffers allocated once: weights; resample count; resample write (its two launches)
    packed   packed.weights + packed.resample: the same with torch.cumsum and the allocations of the result
    torch    the same result from torch ops on the device on a padded (R, n_max) layout: the weights by exp and cumsum, the masses'
             cumsum, searchsorted of the stratified queries, and the gathers of t, deltas and the prefixes; its source rows must equal
             the kernels' on all but the queries that fall within rounding of a prefix: checked before anything is timed.
    roof     the byte model over the HBM rate of DESIGN.md section 5 (8 TB/s): weights 8 B read + 4 B written per row; count 4 B read
             + 4 B written per row; write 40 B written per new row (t, deltas, xyz, dirs, ray_idx, src_row) and 16 B read per source row
             (weights, cdf, t, deltas: once through the caches); per ray 44 B (two (start, count), new_start, mass, origin, dir).  The
             binary searches re-read the prefixes through the caches and are not counted.
  scene    the sphere scene of the README's quick start (rays from (0, 0, -0.5) around +z through the hash field's box, a ball of density
           from tools/bench_occgrid.py's ball_tables): hashfield.render_packed_resampled at the coarse step --coarse-dt with --n-imp
           resampled rows against hashfield.render_packed at --fine-dt, both against render_packed at --ref-dt: rows that go through
           the differentiable field, and the PSNR of rgb * mask against that reference.
Times are device-event medians of 5 repetitions after a warm-up of every shape; nothing here is asserted anywhere and no ratio or image
quality is promised.

    python tools/bench_packed_resample.py [--out profiles/packed_resample.json] [--rays 262144] [--rows 40 80] [--n-imp 32]
"""
import argparse
import json
import math
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_occgrid import ball_tables, clock_state, timed  # noqa: E402

HBM_BYTES_PER_S = 8e12
EPS = 1e-5


def make_list(R, n, seed, dev):
    """a packed list without gaps: counts uniform in [n / 2, 3 n / 2], row p of a ray at t = (p + 0.5) / 64, deltas 1 / 64, unit directions;
    density: a bump of height 60 and width 3 rows around a random row of every ray over a floor of 0.5"""
    g = torch.Generator(device=dev).manual_seed(seed)
    count = torch.randint(n // 2, 3 * n // 2 + 1, (R,), generator=g, device=dev, dtype=torch.int32)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count
    P = int(count.sum())
    ray = torch.repeat_interleave(torch.arange(R, device=dev, dtype=torch.int32), count.long())
    place = (torch.arange(P, device=dev, dtype=torch.int32) - start[ray.long()]).float()
    peak = (torch.rand(R, generator=g, device=dev) * count.float())[ray.long()]
    density = 0.5 + 60.0 * torch.exp(-0.5 * ((place - peak) / 3.0) ** 2)
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g, device=dev), dim=-1)
    return types.SimpleNamespace(t=(place + 0.5) / 64.0, deltas=torch.full((P,), 1.0 / 64.0, device=dev), ray_start=start, ray_count=count, ray_idx=ray,
                                 place=place.long(), density=density, origin=torch.zeros(R, 3, device=dev), dir=d, P=P)


def psnr(x, ref):
    return float(-10.0 * torch.log10(((x - ref) ** 2).mean().clamp_min(1e-20)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_resample.json"))
    ap.add_argument("--rays", type=int, default=1 << 18)
    ap.add_argument("--rows", type=int, nargs="+", default=[40, 80])
    ap.add_argument("--n-imp", type=int, default=32)
    ap.add_argument("--scene-rays", type=int, default=1 << 15)
    ap.add_argument("--coarse-dt", type=float, default=1 / 64)
    ap.add_argument("--fine-dt", type=float, default=1 / 256)
    ap.add_argument("--ref-dt", type=float, default=1 / 1024)
    ap.add_argument("--ibeta", type=float, default=400.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_packed_resample.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, hashfield, mlp, occgrid, packed
    _lib.lib()
    R, n_imp = a.rays, a.n_imp
    aabb = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], device=dev)
    result = {"workload": "weights and inverse-CDF resampling of a packed list of %d rays into %d rows per ray" % (R, n_imp),
              "hbm_bytes_per_s_of_the_roof": HBM_BYTES_PER_S, "clock_state": {"before": clock_state()}, "shapes": {}}
    for n in a.rows:
        L = make_list(R, n, 10 + n, dev)
        P, n_max = L.P, int(L.ray_count.max())
        total = R * n_imp
        u = (torch.arange(n_imp, device=dev, dtype=torch.float32) + 0.5) / n_imp

        def torch_path():
            pad = torch.zeros(R, n_max, device=dev)
            tau = pad.clone()
            tau[L.ray_idx.long(), L.place] = L.density * L.deltas
            excl = torch.cumsum(tau, 1) - tau
            w = (1 - torch.exp(-tau)) * torch.exp(-excl)
            m = torch.where(torch.arange(n_max, device=dev)[None, :] < L.ray_count[:, None], w + EPS, pad)
            C = torch.cumsum(m, 1)
            q = u[None, :] * C[:, -1:]
            i = torch.minimum(torch.searchsorted(C, q.contiguous(), right=True), (L.ray_count[:, None] - 1).long())
            E = torch.gather(C - m, 1, i)
            mi = torch.gather(m, 1, i)
            row = L.ray_start[:, None].long() + i
            f = ((q - E) / mi).clamp(0, 1)
            t = torch.cummax(L.t[row] + (f - 0.5) * L.deltas[row], 1).values
            span = torch.minimum(L.deltas[row], L.deltas[row] * C[:, -1:] / (n_imp * mi))
            return row, t, span, L.origin[:, None, :] + t[..., None] * L.dir[:, None, :]

        w = packed.weights(L.density, L.deltas, L)
        fine = packed.resample(L, w, L.origin, L.dir, n_imp, aabb=aabb, eps=EPS)
        row_torch, t_torch = torch_path()[:2]
        assert int(fine.total) == total == fine.cap and not bool(fine.overflow)
        same_row = float((fine.src_row.long() == row_torch.reshape(-1)).float().mean())
        t_diff = float((fine.t - t_torch.reshape(-1)).abs().max())
        assert same_row > 0.999 and t_diff < 1e-3, (same_row, t_diff)
        # the library's calls alone
        wb, cdf, mass = torch.empty(P, device=dev), torch.empty(P, device=dev), torch.empty(R, device=dev)
        count = torch.empty(R, dtype=torch.int32, device=dev)
        ob = {"t": torch.empty(total, device=dev), "deltas": torch.empty(total, device=dev), "xyz": torch.empty(total, 3, device=dev),
              "dirs": torch.empty(total, 3, device=dev), "ray_idx": torch.empty(total, dtype=torch.int32, device=dev),
              "src_row": torch.empty(total, dtype=torch.int32, device=dev), "ray_count": torch.empty(R, dtype=torch.int32, device=dev),
              "total": torch.empty(1, dtype=torch.int32, device=dev), "overflow": torch.empty(1, dtype=torch.uint8, device=dev)}

        def k_weights():
            _lib.call("packed_weights", L.density, L.deltas, L.ray_start, L.ray_count, R, P, wb, None)

        def k_count():
            _lib.call("packed_resample_count", w, L.ray_start, L.ray_count, R, P, n_imp, EPS, cdf, mass, count)

        def k_write():
            _lib.call("packed_resample_write", w, cdf, mass, L.t, L.deltas, L.ray_start, L.ray_count, fine.ray_start, R, P, L.origin, L.dir, None, n_imp, EPS, total,
                      aabb, ob["t"], ob["deltas"], ob["xyz"], ob["dirs"], ob["ray_idx"], ob["src_row"], ob["ray_count"], ob["total"], ob["overflow"])

        paths = {"packed.weights + packed.resample (three kernels, cumsum, allocations)":
                 lambda: packed.resample(L, packed.weights(L.density, L.deltas, L), L.origin, L.dir, n_imp, aabb=aabb, eps=EPS),
                 "weights kernel": k_weights, "resample count kernel": k_count, "resample write call (write, park)": k_write,
                 "torch: exp, two cumsums, searchsorted and the gathers on the padded (R, n_max) layout": torch_path}
        for fn in paths.values():  # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        times = {k: timed(fn) for k, fn in paths.items()}
        model_bytes = {"weights kernel": 12 * P + 8 * R, "resample count kernel": 8 * P + 16 * R, "resample write call (write, park)": 40 * total + 16 * P + 44 * R}
        kernels_ms = sum(times[k]["median_ms"] for k in model_bytes)
        roof_ms = {k: v / HBM_BYTES_PER_S * 1e3 for k, v in model_bytes.items()}
        keys = list(paths)
        result["shapes"]["about %d rows per ray" % n] = {
            "rays": R, "rows": P, "n_max": n_max, "new_rows": total, "times": times, "source_rows_equal_to_the_torch_path": round(same_row, 6), "max_abs_t_difference_to_the_torch_path": t_diff,
            "kernels": {k: {"model_bytes": model_bytes[k], "roof_ms": round(roof_ms[k], 4), "share_of_the_byte_roof": round(roof_ms[k] / times[k]["median_ms"], 3)}
                        for k in model_bytes},
            "three_kernels_ms": round(kernels_ms, 4), "torch_over_three_kernels": round(times[keys[4]]["median_ms"] / kernels_ms, 2),
            "torch_over_packed": round(times[keys[4]]["median_ms"] / times[keys[0]]["median_ms"], 2)}
        del L, w, fine, wb, cdf, mass, count, ob, row_torch, t_torch
        torch.cuda.empty_cache()
    # ---- the sphere scene ----
    Rs = a.scene_rays
    P, cfg = hashfield.make_weights(0, sdf_bias=0.02)
    ball_tables(P, cfg)
    P["logibeta"] = torch.tensor([math.log(a.ibeta)])
    P = {k: v.to(dev) for k, v in P.items()}
    g = torch.Generator(device=dev).manual_seed(1)
    o = torch.tensor([[0.0, 0.0, -0.5]], device=dev).repeat(Rs, 1)
    d = torch.nn.functional.normalize(torch.randn(Rs, 3, generator=g, device=dev) * 0.1 + torch.tensor([0.0, 0.0, 1.0], device=dev), dim=-1)
    tr = torch.tensor([[0.0, 1.0]], device=dev).repeat(Rs, 1)
    hres = hashfield.resolutions(cfg, dev)
    grid = hashfield.update_occupancy(P, cfg, occgrid.OccupancyGrid(P["aabb"], G=128))
    scene = {"rays": Rs, "n_imp": n_imp, "coarse_dt": a.coarse_dt, "fine_dt": a.fine_dt, "reference_dt": a.ref_dt, "ibeta": a.ibeta}
    with torch.no_grad():
        def fixed(dt):
            k_max = int(math.ceil(1.0 / dt)) + 1
            total = int(packed.march(grid, o, d, tr, dt, 0, k_max=k_max).total)
            rgb, mask, depth, tot, ovf = hashfield.render_packed(P, cfg, grid, o, d, tr, dt, total + 64, k_max=k_max, res=hres)
            assert not bool(ovf)
            return rgb, mask, depth, int(tot)

        ref = fixed(a.ref_dt)
        fine_fixed = fixed(a.fine_dt)
        k_max = int(math.ceil(1.0 / a.coarse_dt)) + 1
        coarse_total = int(packed.march(grid, o, d, tr, a.coarse_dt, 0, k_max=k_max).total)
        rs = hashfield.render_packed_resampled(P, cfg, grid, o, d, tr, a.coarse_dt, coarse_total + 64, n_imp, k_max=k_max, res=hres)
        assert not bool(rs[4]) and not bool(rs[6])
        coarse_fixed = fixed(a.coarse_dt)
        for name, out, rows, extra in (("render_packed at the fine step", fine_fixed, fine_fixed[3], 0), ("render_packed at the coarse step", coarse_fixed, coarse_fixed[3], 0),
                                       ("render_packed_resampled: coarse step + n_imp rows", rs, int(rs[5]), coarse_total)):
            scene[name] = {"rows_through_the_differentiable_field": rows, "rows_through_the_density_pass_without_gradients": extra,
                           "psnr_rgb_db": round(psnr(out[0], ref[0]), 2), "psnr_mask_db": round(psnr(out[1], ref[1]), 2), "psnr_depth_db": round(psnr(out[2], ref[2]), 2)}
        scene["reference_rows"] = ref[3]
    result["scene"] = scene
    result["clock_state"]["after"] = clock_state()
    result["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
