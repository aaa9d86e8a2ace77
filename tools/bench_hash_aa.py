"""Cost of the footprint-weighted hash encoding (hashgrid.hash_encode(radius=..., w_min=...)) on one GPU: forward + backward
with the table gradient at S = 2^22 samples on the bench's table (hashfield.DEFAULT), timed with device events, medians of alternating rounds.

  (a) hash_encode()                              the unweighted kernels, as before the feature
  (b) hash_encode(radius = 0)                    the weighted instantiations on point samples: the price of the instantiation itself
  (c) hash_encode(radius = cone-like, w_min)     radius = t * footprint, t uniform in [t_near, t_far] in box edges, sorted in runs of 256
                                                 samples like the rows of a ray; reported with the share of (sample, level) pairs whose weight is 0
  (d) hash_encode() * level_weights(...)         the composition in torch: the same values without any skip

    python tools/bench_hash_aa.py [--log2-s 22] [--rounds 7] [--f16]

Prints one JSON line.  Needs the GPU: there is no CPU timing."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lab4d_amd import hashfield, hashgrid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-s", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--w-min", type=float, default=1.0 / 256)
    ap.add_argument("--footprint", type=float, default=0.05, help="Gaussian radius per unit of distance, in box edges")
    ap.add_argument("--t-near", type=float, default=0.5)
    ap.add_argument("--t-far", type=float, default=8.0)
    ap.add_argument("--f16", action="store_true", help="the packed-fp16 table gradient on the hashed levels (what bench.py --config hash runs)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hash_aa: needs the GPU (a CPU run measures nothing)")
    dev, cfg = "cuda", dict(hashfield.DEFAULT)
    S, L, F = 1 << a.log2_s, cfg["L"], cfg["F"]
    g = torch.Generator().manual_seed(0)
    res_l = hashgrid.level_resolutions(L, cfg["n_min"], cfg["n_max"])
    res = torch.tensor(res_l, dtype=torch.int32, device=dev)
    f16_from = hashgrid.first_hashed_level(res_l, cfg["log2_T"]) if a.f16 else None
    table = ((torch.rand(L, 1 << cfg["log2_T"], F, generator=g) * 2 - 1) * 1e-1).to(dev).requires_grad_(True)
    # rows of rays: runs of 256 consecutive samples along a segment through the cube, t ascending within the run
    n_rays = S // 256
    p0, p1 = torch.rand(n_rays, 1, 3, generator=g), torch.rand(n_rays, 1, 3, generator=g)
    u = torch.linspace(0, 1, 256)[None, :, None]
    x = (p0 + (p1 - p0) * u).reshape(S, 3).to(dev).contiguous()
    t0 = a.t_near + (a.t_far - a.t_near) * torch.rand(n_rays, 1, generator=g)
    t = (t0 + torch.linspace(0, 1, 256)[None, :] * 0.5).reshape(S).to(dev)
    radius = (t * a.footprint).contiguous()
    zeros = torch.zeros(S, device=dev)
    cot = torch.randn(S, L * F, generator=g).to(dev)
    share_zero = float((hashgrid.level_weights(radius, res, a.w_min) == 0).float().mean())

    def step(kind):
        table.grad = None
        if kind == "a":
            out = hashgrid.hash_encode(x, table, res, cfg["log2_T"], inside_only=True, f16_from=f16_from)
        elif kind == "b":
            out = hashgrid.hash_encode(x, table, res, cfg["log2_T"], inside_only=True, f16_from=f16_from, radius=zeros, w_min=a.w_min)
        elif kind == "c":
            out = hashgrid.hash_encode(x, table, res, cfg["log2_T"], inside_only=True, f16_from=f16_from, radius=radius, w_min=a.w_min)
        else:
            out = hashgrid.hash_encode(x, table, res, cfg["log2_T"], inside_only=True, f16_from=f16_from)
            out = out * hashgrid.level_weights(radius, res, a.w_min).repeat_interleave(F, -1)
        (out * cot).sum().backward()

    kinds = ("a", "b", "c", "d")
    times = {k: [] for k in kinds}
    for r in range(a.warmup + a.rounds):
        for k in kinds:  # alternating: every round times every variant once
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            step(k)
            e.record()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[k].append(s.elapsed_time(e))
    # the variants compute the same thing where they should
    with torch.no_grad():
        n = 1 << 16
        oa = hashgrid.hash_encode(x[:n], table, res, cfg["log2_T"], inside_only=True)
        ob = hashgrid.hash_encode(x[:n], table, res, cfg["log2_T"], inside_only=True, radius=zeros[:n], w_min=a.w_min)
        oc = hashgrid.hash_encode(x[:n], table, res, cfg["log2_T"], inside_only=True, radius=radius[:n], w_min=a.w_min)
        od = oa * hashgrid.level_weights(radius[:n], res, a.w_min).repeat_interleave(F, -1)
        same = {"b_equals_a": bool(torch.equal(oa, ob)), "c_minus_d_max": float((oc - od).abs().max()), "out_max": float(od.abs().max())}
    out = {"tool": "bench_hash_aa", "S": S, "cfg": cfg, "f16_from": f16_from, "w_min": a.w_min, "footprint": a.footprint, "t": [a.t_near, a.t_far + 0.5],
           "share_of_zero_weights": round(share_zero, 4), "rounds": a.rounds, "check": same}
    for k in kinds:
        out["ms_" + k] = {"median": round(statistics.median(times[k]), 3), "min": round(min(times[k]), 3), "max": round(max(times[k]), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
