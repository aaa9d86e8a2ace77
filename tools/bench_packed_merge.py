"""Merge of two packed sample lists per ray (include/lab4d_pmerge.h), measured: R rays with about n rows per ray in EACH list (counts uniform
in [n / 2, 3 n / 2], no gaps, t ascending within a ray on two interleaving lattices with jitter), for every n of --rows.
    merge    packed.merge: the count kernel, torch.cumsum, the write call (clear + write + park) and the allocations of the result
    kernels  the library's calls alone on buffers allocated once: count; write (its three launches); one gather of C = 3 channels
    torch    the same result from torch ops on the device: the concatenation sorted by t and then by ray, both sorts stable
             (src = order_t[order_ray]), and the index gathers of t, deltas, ray_idx; and a[src] of C = 3 channels for the gather.
             Its src must equal the kernels': checked before anything is timed.
    roof     the byte model over the HBM rate of DESIGN.md section 5 (8 TB/s): per input row 8 B read (t, deltas), 4 B of pos cleared and
             4 B written, 16 B of merged row written (t, deltas, ray_idx, src); per ray 20 B read (two (start, count), ray_start) and 8 B
             written in the two passes.  The binary searches re-read t of the other list through the caches and are not counted.  The
             gather: 4 B of idx, 4 C B read and 4 C B written per row.
Times are device-event medians of 5 repetitions after a warm-up of every shape; nothing here is asserted anywhere and no ratio is promised.

    python tools/bench_packed_merge.py [--out profiles/packed_merge.json] [--rays 262144] [--rows 40 80]
"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_occgrid import clock_state, timed  # noqa: E402

HBM_BYTES_PER_S = 8e12


def make_list(R, n, step, seed, dev):
    """a packed list without gaps: counts uniform in [n / 2, 3 n / 2], row p of a ray at t = (p + u) * step, u uniform in [0, 1)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    count = torch.randint(n // 2, 3 * n // 2 + 1, (R,), generator=g, device=dev, dtype=torch.int32)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count
    P = int(count.sum())
    ray = torch.repeat_interleave(torch.arange(R, device=dev, dtype=torch.int32), count.long())
    place = torch.arange(P, device=dev, dtype=torch.int32) - start[ray.long()]
    t = (place.float() + torch.rand(P, generator=g, device=dev)) * step
    return types.SimpleNamespace(t=t, deltas=torch.full((P,), step, device=dev), ray_start=start, ray_count=count, ray_idx=ray, P=P)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_merge.json"))
    ap.add_argument("--rays", type=int, default=1 << 18)
    ap.add_argument("--rows", type=int, nargs="+", default=[40, 80])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_packed_merge.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, packed
    _lib.lib()
    R, C = a.rays, 3
    result = {"workload": "merge of two packed lists of %d rays, counts uniform in [n / 2, 3 n / 2] per list, and one gather of %d channels" % (R, C),
              "hbm_bytes_per_s_of_the_roof": HBM_BYTES_PER_S, "clock_state": {"before": clock_state()}, "shapes": {}}
    for n in a.rows:
        A, B = make_list(R, n, 1.0, 10 + n, dev), make_list(R, n, 0.7, 20 + n, dev)
        Pa, Pb = A.P, B.P
        total = Pa + Pb
        va, vb = torch.rand(Pa, C, device=dev), torch.rand(Pb, C, device=dev)
        t_cat, d_cat, ray_cat, v_cat = torch.cat([A.t, B.t]), torch.cat([A.deltas, B.deltas]), torch.cat([A.ray_idx, B.ray_idx]), torch.cat([va, vb])

        def torch_merge():
            order_t = torch.sort(t_cat, stable=True).indices
            src = order_t[torch.sort(ray_cat[order_t], stable=True).indices]
            return src, t_cat[src], d_cat[src], ray_cat[src]

        merged = packed.merge(A, B)
        src_torch = torch_merge()[0]
        assert int(merged.total) == total == merged.cap and not bool(merged.overflow)
        assert torch.equal(merged.src.long(), src_torch), "the torch path and the kernels disagree on src"
        assert torch.equal(packed.merge_rows(merged, va, vb), v_cat[src_torch])
        # the library's calls alone
        count = torch.empty(R, dtype=torch.int32, device=dev)
        ob = {"t": torch.empty(total, device=dev), "deltas": torch.empty(total, device=dev), "ray_idx": torch.empty(total, dtype=torch.int32, device=dev),
              "src": torch.empty(total, dtype=torch.int32, device=dev), "pos_a": torch.empty(Pa, dtype=torch.int32, device=dev),
              "pos_b": torch.empty(Pb, dtype=torch.int32, device=dev), "ray_count": torch.empty(R, dtype=torch.int32, device=dev),
              "total": torch.empty(1, dtype=torch.int32, device=dev), "overflow": torch.empty(1, dtype=torch.uint8, device=dev)}
        out = torch.empty(total, C, device=dev)

        def k_count():
            _lib.call("packed_merge_count", A.ray_start, A.ray_count, Pa, B.ray_start, B.ray_count, Pb, R, count)

        def k_write():
            _lib.call("packed_merge_write", A.t, A.deltas, A.ray_start, A.ray_count, Pa, B.t, B.deltas, B.ray_start, B.ray_count, Pb, R, merged.ray_start, total,
                      ob["t"], ob["deltas"], ob["ray_idx"], ob["src"], ob["pos_a"], ob["pos_b"], ob["ray_count"], ob["total"], ob["overflow"])

        def k_gather():
            _lib.call("packed_merge_gather", va, Pa, vb, Pb, merged.src, total, C, out)

        paths = {"packed.merge (count, cumsum, write, allocations)": lambda: packed.merge(A, B), "count kernel": k_count,
                 "write call (clear, write, park)": k_write, "gather kernel, C = 3": k_gather,
                 "torch: two stable sorts and the gathers of t, deltas, ray_idx": torch_merge, "torch: index gather, C = 3": lambda: v_cat[src_torch]}
        for fn in paths.values():  # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        times = {k: timed(fn) for k, fn in paths.items()}
        merge_bytes = 32 * total + 28 * R
        gather_bytes = (4 + 8 * C) * total
        roof_merge_ms, roof_gather_ms = merge_bytes / HBM_BYTES_PER_S * 1e3, gather_bytes / HBM_BYTES_PER_S * 1e3
        kernels_ms = times["count kernel"]["median_ms"] + times["write call (clear, write, park)"]["median_ms"]
        merge_ms, gather_ms = times["packed.merge (count, cumsum, write, allocations)"]["median_ms"], times["gather kernel, C = 3"]["median_ms"]
        torch_ms, torch_gather_ms = (times["torch: two stable sorts and the gathers of t, deltas, ray_idx"]["median_ms"],
                                     times["torch: index gather, C = 3"]["median_ms"])
        result["shapes"]["about %d rows per ray and list" % n] = {
            "rays": R, "rows_a": Pa, "rows_b": Pb, "times": times,
            "merge": {"median_ms": merge_ms, "torch_over_merge": round(torch_ms / merge_ms, 2), "model_bytes": merge_bytes, "roof_ms": round(roof_merge_ms, 4),
                      "share_of_the_byte_roof": round(roof_merge_ms / merge_ms, 3), "share_of_the_byte_roof_kernels_alone": round(roof_merge_ms / kernels_ms, 3)},
            "gather": {"median_ms": gather_ms, "torch_over_gather": round(torch_gather_ms / gather_ms, 2), "model_bytes": gather_bytes,
                       "roof_ms": round(roof_gather_ms, 4), "share_of_the_byte_roof": round(roof_gather_ms / gather_ms, 3)}}
        del A, B, merged, ob, out, va, vb, t_cat, d_cat, ray_cat, v_cat, src_torch
        torch.cuda.empty_cache()
    result["clock_state"]["after"] = clock_state()
    result["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
