"""The proposal loss between two packed lists and the weights adjoint (include/lab4d_proposal.h), measured.
  timing   R rays; an envelope list of about n rows per ray (counts uniform in [n / 2, 3 n / 2], no gaps, unit directions, a random density
           with a peak somewhere along every ray) and the fine list that packed.resample makes of it with n_imp rows per ray, whose
           weights come from a second density of the same shape:
    kernels  the library's calls alone on buffers allocated once: weights adjoint; envelope; proposal forward; proposal backward.  The
             backward walks n_f * ceil(n_e / 64) steps per ray with the whole wave: its time is reported here, nobody had measured it.
    packed   packed.render_weights + packed.proposal_loss + backward through autograd: the same with the allocations
    torch    the same result from torch ops on the device on a padded layout: the weights by exp and cumsum on (R, n_max), the intervals,
             two searchsorted, the prefix differences, the loss, and autograd's backward through all of it.  Its summed loss must agree
             with the kernels' to 1e-3 relative and its gradient to 1e-2 in the L2 norm (an interval end that rounds differently moves a
             touching pair in or out of a span, so single rays may differ by a whole weight): checked before anything is timed.
Times are device-event medians of 5 repetitions after a warm-up of every shape; nothing here is asserted anywhere and no ratio is promised.

    python tools/bench_packed_proposal.py [--out profiles/packed_proposal.json] [--rays 262144] [--rows 40] [--n-imp 32]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_occgrid import clock_state, timed  # noqa: E402
from bench_packed_resample import make_list  # noqa: E402

EPS = float(torch.finfo(torch.float32).eps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_proposal.json"))
    ap.add_argument("--rays", type=int, default=1 << 18)
    ap.add_argument("--rows", type=int, nargs="+", default=[40])
    ap.add_argument("--n-imp", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_packed_proposal.py measures on the GPU; none found (there is no CPU path)")
    dev = torch.device("cuda", 0)
    from lab4d_amd import _lib, packed
    _lib.lib()
    R, n_imp = a.rays, a.n_imp
    aabb = torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], device=dev)
    result = {"workload": "proposal loss of %d rays: an envelope list against a fine list of %d rows per ray, forward and adjoint, with the weights adjoint" % (R, n_imp),
              "clock_state": {"before": clock_state()}, "shapes": {}}
    for n in a.rows:
        L = make_list(R, n, 10 + n, dev)
        Pe, n_max = L.P, int(L.ray_count.max())
        with torch.no_grad():
            fine = packed.resample(L, packed.weights(L.density, L.deltas, L), L.origin, L.dir, n_imp, aabb=aabb, eps=1e-5)
            w_f = packed.weights(60.0 * torch.rand(fine.cap, device=dev, generator=torch.Generator(device=dev).manual_seed(n)), fine.deltas, fine)
        Pf = fine.cap
        g_loss = torch.full((R,), 1.0 / R, device=dev)
        place_f = (torch.arange(Pf, device=dev) - fine.ray_start[fine.ray_idx.long()].long())

        def packed_path():
            dens = L.density.clone().requires_grad_(True)
            w = packed.render_weights(dens, L.deltas, L)
            loss = packed.proposal_loss(L, w, fine, w_f, L.dir, eps=EPS)
            (loss * g_loss).sum().backward()
            return loss.detach(), dens.grad

        def torch_path():
            dens = L.density.clone().requires_grad_(True)
            live = torch.arange(n_max, device=dev)[None, :] < L.ray_count[:, None]
            tau = torch.zeros(R, n_max, device=dev).index_put((L.ray_idx.long(), L.place), dens * L.deltas)
            w = (1 - torch.exp(-tau)) * torch.exp(-(torch.cumsum(tau, 1) - tau))
            inf = torch.full((R, n_max), float("inf"), device=dev)
            t = inf.index_put((L.ray_idx.long(), L.place), L.t)
            h = torch.zeros(R, n_max, device=dev).index_put((L.ray_idx.long(), L.place), 0.5 * L.deltas)  # (unit directions)
            lo_e, hi_e = torch.where(live, t - h, inf), torch.where(live, t + h, inf)
            C = torch.nn.functional.pad(torch.cumsum(torch.where(live, w.clamp_min(0), torch.zeros_like(w)), 1), (1, 0))
            lo = (fine.t - 0.5 * fine.deltas).reshape(R, n_imp)
            hi = (fine.t + 0.5 * fine.deltas).reshape(R, n_imp)
            j0 = torch.searchsorted(hi_e, lo.contiguous(), right=True)
            j1 = torch.searchsorted(lo_e, hi.contiguous(), right=False)
            B = torch.where(j1 > j0, torch.gather(C, 1, j1) - torch.gather(C, 1, j0), torch.zeros_like(lo))
            v = w_f.reshape(R, n_imp).clamp_min(0)
            x = (v - B).clamp_min(0)
            loss = (x * x / (v + EPS)).sum(1)
            (loss * g_loss).sum().backward()
            return loss.detach(), dens.grad

        assert int(fine.total) == R * n_imp == Pf and place_f.max() < n_imp
        (loss_k, grad_k), (loss_t, grad_t) = packed_path(), torch_path()
        loss_diff = float((loss_k.double().sum() - loss_t.double().sum()).abs() / loss_t.double().sum())
        grad_diff = float((grad_k - grad_t).double().norm() / grad_t.double().norm())
        assert loss_diff < 1e-3 and grad_diff < 1e-2, (loss_diff, grad_diff)
        # the library's calls alone
        w = packed.weights(L.density, L.deltas, L)
        lo_b, hi_b, cdf_b, g_w_e, g_dens = (torch.zeros(Pe, device=dev) for _ in range(5))
        span, coef, loss_b = torch.zeros(Pf, 2, dtype=torch.int32, device=dev), torch.zeros(Pf, device=dev), torch.zeros(R, device=dev)

        def k_envelope():
            _lib.call("packed_envelope", w, L.t, L.deltas, L.ray_start, L.ray_count, L.dir, R, Pe, lo_b, hi_b, cdf_b)

        def k_forward():
            _lib.call("packed_proposal_forward", lo_b, hi_b, cdf_b, L.ray_start, L.ray_count, Pe, w_f, fine.t, fine.deltas, fine.ray_start, fine.ray_count, Pf, L.dir, R,
                      EPS, span, coef, loss_b)

        def k_backward():
            _lib.call("packed_proposal_backward", g_loss, span, coef, w, L.ray_start, L.ray_count, Pe, fine.ray_start, fine.ray_count, Pf, R, g_w_e)

        def k_weights_backward():
            _lib.call("packed_weights_backward", L.density, L.deltas, L.ray_start, L.ray_count, R, Pe, g_w_e, None, g_dens)

        paths = {"packed.render_weights + packed.proposal_loss + backward (five kernels, allocations, autograd)": packed_path,
                 "envelope kernel": k_envelope, "proposal forward kernel": k_forward, "proposal backward kernel": k_backward,
                 "weights adjoint kernel": k_weights_backward,
                 "torch: exp, cumsums, two searchsorted, gathers and autograd's backward on the padded (R, n_max) layout": torch_path}
        for fn in paths.values():  # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        times = {k: timed(fn) for k, fn in paths.items()}
        keys = list(paths)
        kernels_ms = sum(times[k]["median_ms"] for k in keys[1:5])
        steps = float((fine.ray_count.float() * torch.ceil(L.ray_count.float() / 64)).sum())
        result["shapes"]["about %d rows per ray" % n] = {
            "rays": R, "envelope_rows": Pe, "n_max": n_max, "fine_rows": Pf, "times": times, "relative_difference_of_the_summed_loss_to_the_torch_path": loss_diff,
            "relative_l2_difference_of_the_gradient_to_the_torch_path": grad_diff, "four_kernels_ms": round(kernels_ms, 4),
            "backward_loop_steps": steps, "backward_ns_per_wave_step": round(times[keys[3]]["median_ms"] * 1e6 / steps, 3),
            "torch_over_packed": round(times[keys[5]]["median_ms"] / times[keys[0]]["median_ms"], 2)}
    result["clock_state"]["after"] = clock_state()
    result["device"] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
