"""The proposal loss between two packed lists and the weights adjoint on the device (csrc/proposal.hip through lab4d_amd/packed.py and
hashfield.render_packed_proposal): the envelope, forward and backward kernels against the CPU twin
(tests/host_harness/proposal/proposal_host.cpp) WORD FOR WORD, the weights adjoint against float64 autograd, both autograd Functions against
the float64 references, then render_packed_proposal -- where the gradients go, and that a proposal field learns -- and graph capture."""
import functools
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proposal_checks as PR  # noqa: E402

from lab4d_amd import _lib, hashfield, mlp, occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_loss(case, eps=PR.EPS, g_loss=None):
    """the library's three calls on buffers pre-filled with the sentinels of PR.host_loss -> its dict"""
    e, f, R = case["e"], case["f"], case["R"]
    de, df = ({k: dev(lst[k]) for k in ("w", "t", "deltas", "start", "count")} for lst in (e, f))
    d = dev(case["dir"])
    out = {k: torch.full((e["P"],), float(PR.SENTINEL_F), device=DEV) for k in ("lo_e", "hi_e", "cdf_e", "g_w_e")}
    out.update(span=torch.full((f["P"], 2), int(PR.SENTINEL_I), dtype=torch.int32, device=DEV), coef=torch.full((f["P"],), float(PR.SENTINEL_F), device=DEV),
               loss=torch.full((R,), float(PR.SENTINEL_F), device=DEV))
    _lib.call("packed_envelope", de["w"], de["t"], de["deltas"], de["start"], de["count"], d, R, e["P"], out["lo_e"], out["hi_e"], out["cdf_e"])
    _lib.call("packed_proposal_forward", out["lo_e"], out["hi_e"], out["cdf_e"], de["start"], de["count"], e["P"], df["w"], df["t"], df["deltas"], df["start"],
              df["count"], f["P"], d, R, eps, out["span"], out["coef"], out["loss"])
    g = dev(PR.g_loss_of(R) if g_loss is None else g_loss)
    _lib.call("packed_proposal_backward", g, out["span"], out["coef"], de["w"], de["start"], de["count"], e["P"], df["start"], df["count"], f["P"], R, out["g_w_e"])
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_kernels_equal_the_cpu_twin_word_for_word():
    """the lists of tests/proposal_checks.py at R = 1025 (every pairing of the lengths 0 / 1 / 2 / 63 / 64 / 65 / 129 / 200, gaps, a
    (start, count) that leaves [0, P), |dir| = 0, weights with zeros, a NaN and a negative value), eps = 2^-23 and 0: every output array of
    the three kernels; the sentinels show what was left alone"""
    lib = PR.build_host()
    case = PR.make_case(1025, seed=1725)
    for eps in (PR.EPS, 0.0):
        got, ref = device_loss(case, eps), PR.host_loss(lib, case, eps)
        PR.assert_same(got, ref, eps)
        free = ~PR.owned(case["e"], 1025)
        assert free.sum() > 20 and (got["g_w_e"][free] == PR.SENTINEL_F).all() and (got["span"][~PR.owned(case["f"], 1025)] == PR.SENTINEL_I).all()
        assert np.isfinite(got["loss"]).all() and got["loss"].max() > 1


def test_every_wave_runs_several_rays():
    """66,000 short rays: more than the 4 x 16,384 rays that one pass of the largest grid takes, so the first blocks' waves come round again"""
    lib = PR.build_host()
    rng = np.random.default_rng(8)
    R = 66000
    case = {"R": R, "dir": rng.standard_normal((R, 3)).astype(np.float32)}
    length = PR.dir_length(case["dir"])
    for key in ("e", "f"):
        count = rng.choice(np.int32([0, 1, 2, 3, 70]), R, p=[0.3, 0.3, 0.2, 0.19, 0.01])
        P = int(count.sum())
        start = (np.cumsum(count) - count).astype(np.int32)
        t = np.zeros(P, np.float32)
        for s, n in zip(start[count > 0], count[count > 0]):
            t[s:s + n] = (np.arange(1, n + 1) + (0.5 if key == "e" else rng.random(n) - 0.5)) / 64.0
        case[key] = {"P": P, "start": start, "count": count, "t": t, "deltas": np.repeat(length / np.float32(64.0 if key == "e" else 128.0), count).astype(np.float32),
                     "w": rng.random(P).astype(np.float32)}
    got, ref = device_loss(case), PR.host_loss(lib, case)
    PR.assert_same(got, ref, "66000 rays")
    assert (got["loss"] > 0).sum() > 20000 and (got["g_w_e"] != 0).sum() > 10000


def test_weights_backward_against_float64_autograd():
    """lab4d_packed_weights_backward against float64 autograd through the oracle's compute_weights ray by ray, at the 1e-4 bar in the metric
    max |x - ref| / max |ref|, with and without g_trans; a NaN, a negative and a zero density get no gradient; the rows of no ray are left
    alone.  Measured maximum on the MI355X: 8.3e-8."""
    lst, density, g_w, g_trans = PR.weights_case()
    R, P = lst["start"].shape[0], lst["P"]
    own = PR.owned(lst, R)
    ref_args = [dev(density), dev(lst["deltas"]), dev(lst["start"]), dev(lst["count"]), R, P, dev(g_w)]
    for gt in (None, g_trans):
        got = torch.full((P,), float(PR.SENTINEL_F), device=DEV)
        _lib.call("packed_weights_backward", *ref_args, None if gt is None else dev(gt), got)
        got = got.cpu().numpy()
        ref = PR.weights_backward64(lst, density, g_w, gt)
        err = PR.rel_err(got[own], ref[own])
        print("packed_weights_backward against float64 autograd (g_trans %s): %.2e" % (gt is not None, err))
        s3, _ = PR.rows_of(lst, 3)
        assert err <= PR.BAR and (got[~own] == PR.SENTINEL_F).all() and got[s3 + 1] == 0 and got[s3 + 2] == 0 and got[s3 + 5] == 0 and np.abs(ref).max() > 1e-2


def _rays(lst):
    return types.SimpleNamespace(t=dev(lst["t"]), deltas=dev(lst["deltas"]), ray_start=dev(lst["start"]), ray_count=dev(lst["count"]))


def test_render_weights_through_autograd():
    """packed.render_weights: its forward is packed.weights bit for bit; the gradient of sum(g_w w) + sum(g_trans trans) that autograd
    returns for the density against the float64 reference at the 1e-4 bar, zeros in the rows of no ray; deltas gets no gradient"""
    lst, density, g_w, g_trans = PR.weights_case()
    R = lst["start"].shape[0]
    rays = _rays(lst)
    dens = dev(density)[:, None].requires_grad_(True)
    deltas = dev(lst["deltas"]).requires_grad_(True)
    w, trans = packed.render_weights(dens, deltas, rays, with_trans=True)
    w0, trans0 = packed.weights(dens, deltas, rays, with_trans=True)
    assert torch.equal(w, w0) and torch.equal(trans, trans0) and w.requires_grad and tuple(w.shape) == (lst["P"],)
    ((w * dev(g_w)).sum() + (trans * dev(g_trans)).sum()).backward()
    own = PR.owned(lst, R)
    got, ref = dens.grad[:, 0].cpu().numpy(), PR.weights_backward64(lst, density, g_w, g_trans)
    err = PR.rel_err(got[own], ref[own])
    print("render_weights through autograd against float64: %.2e" % err)
    assert err <= PR.BAR and (got[~own] == 0).all() and deltas.grad is None
    dens.grad = None
    (packed.render_weights(dens, deltas, rays) * dev(g_w)).sum().backward()  # without trans
    assert PR.rel_err(dens.grad[:, 0].cpu().numpy()[own], PR.weights_backward64(lst, density, g_w)[own]) <= PR.BAR


def test_proposal_loss_through_autograd():
    """packed.proposal_loss: the loss and the gradient autograd returns for w_env against the float64 brute force at the 1e-4 bar, equal to
    the twin word for word; zeros in the rows of no ray; w_fine gets no gradient"""
    lib = PR.build_host()
    R = 1025
    case = PR.make_case(R, seed=1725)
    g = PR.g_loss_of(R)
    w_e = dev(case["e"]["w"])[:, None].requires_grad_(True)
    w_f = dev(case["f"]["w"]).requires_grad_(True)
    loss = packed.proposal_loss(_rays(case["e"]), w_e, _rays(case["f"]), w_f, dev(case["dir"]))
    assert tuple(loss.shape) == (R,) and loss.requires_grad
    (loss * dev(g)).sum().backward()
    twin = PR.host_loss(lib, case, g_loss=g)
    brute = PR.brute64(case, twin, g_loss=g)
    own = PR.owned(case["e"], R)
    got = w_e.grad[:, 0].cpu().numpy()
    errs = {"loss": PR.rel_err(loss.detach().cpu().numpy(), brute["loss"]), "g_w_e": PR.rel_err(got[own], brute["g_w_e"][own])}
    print("proposal_loss through autograd against float64:", {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) <= PR.BAR and w_f.grad is None and (got[~own] == 0).all()
    assert np.array_equal(PR.words(loss.detach().cpu().numpy()), PR.words(twin["loss"])) and np.array_equal(PR.words(got[own]), PR.words(twin["g_w_e"][own]))


# ---------------------------------------------------------------------------------------------------
# the hash field with a proposal field
# ---------------------------------------------------------------------------------------------------
R_SCENE, N_IMP, DT = 4096, 32, 1.0 / 64.0


def ball_field():
    """the main field of the README's sphere scene: a ball of density ~10 of radius 0.25 of the box (level 0 carries 20 (0.3 - r), the
    geometry net passes it through, sdf = 1 - relu(.)), sharpened to ibeta = 400"""
    P, cfg = hashfield.make_weights(0, sdf_bias=0.02)
    for k in ("hash.table", "hash.geo.0.weight", "hash.geo.0.bias", "hash.geo.2.weight", "hash.geo.2.bias"):
        P[k].zero_()
    n = cfg["n_min"] + 1
    ax = torch.arange(n, dtype=torch.float64) / cfg["n_min"] - 0.5
    iz, iy, ix = torch.meshgrid(ax, ax, ax, indexing="ij")
    P["hash.table"][0, :n ** 3, 0] = (20 * (0.3 - torch.sqrt(ix ** 2 + iy ** 2 + iz ** 2))).reshape(-1).float()
    P["hash.geo.0.weight"][0, 0] = 1.0
    P["hash.geo.2.weight"][0, 0] = -1.0
    P["hash.geo.2.bias"][0] = 1.0
    P["logibeta"] = torch.tensor([math.log(400.0)])
    return P, cfg


@functools.lru_cache(None)
def scene():
    """4096 rays from (0, 0, -0.5) around +z through the box of the ball field, its occupancy grid, and a small proposal field (log2_T 12,
    n_max 128) from make_weights"""
    P, cfg = ball_field()
    Pp, cfgp = hashfield.make_weights(3, {"L": 16, "F": 2, "log2_T": 12, "n_min": 16, "n_max": 128})
    g = torch.Generator().manual_seed(1)
    o = torch.tensor([[0.0, 0.0, -0.5]]).repeat(R_SCENE, 1)
    d = torch.nn.functional.normalize(torch.randn(R_SCENE, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, 1.0]), dim=-1)
    tr = torch.tensor([[0.0, 1.0]]).repeat(R_SCENE, 1)
    Pd = {k: v.to(DEV) for k, v in P.items()}
    grid = hashfield.update_occupancy(Pd, cfg, occgrid.OccupancyGrid(Pd["aabb"], G=64))
    cap = int(packed.march(grid, o.to(DEV), d.to(DEV), tr.to(DEV), DT, 0, k_max=65).total) + 64
    return {"P": P, "cfg": cfg, "Pp": Pp, "cfgp": cfgp, "o": o.to(DEV), "d": d.to(DEV), "tr": tr.to(DEV), "grid": grid, "cap": cap}


def _leaves(P):
    return {k: v.to(DEV).clone().requires_grad_(k != "aabb") for k, v in P.items()}


def _render(sc, Pp, P):
    return hashfield.render_packed_proposal(Pp, sc["cfgp"], P, sc["cfg"], sc["grid"], sc["o"], sc["d"], sc["tr"], DT, sc["cap"], N_IMP, prec=mlp.PREC_F32, k_max=65)


def test_render_packed_proposal_routes_the_gradients():
    """outputs finite, prop_loss >= 0 and somewhere > 0; prop_loss.mean().backward() reaches the proposal field's table and leaves the
    main field without gradients; rgb.sum().backward() does the reverse"""
    sc = scene()
    Pp, P = _leaves(sc["Pp"]), _leaves(sc["P"])
    out = _render(sc, Pp, P)
    rgb, mask, depth, total, ovf, total_fine, ovf_fine, prop = out
    assert len(out) == 8 and tuple(rgb.shape) == (R_SCENE, 3) and tuple(prop.shape) == (R_SCENE, 1) and tuple(mask.shape) == tuple(depth.shape) == (R_SCENE, 1)
    for k, x in zip(("rgb", "mask", "depth", "prop_loss"), (rgb, mask, depth, prop)):
        assert bool(torch.isfinite(x).all()), k
    assert int(total) > 1000 and not bool(ovf) and not bool(ovf_fine) and int(total_fine) % N_IMP == 0 and int(total_fine) > 0
    assert bool((prop >= 0).all()) and float(prop.detach().max()) > 0 and float(mask.detach().max()) > 0.5
    prop.mean().backward(retain_graph=True)
    assert float(Pp["hash.table"].grad.abs().max()) > 0 and bool(torch.isfinite(Pp["hash.table"].grad).all())
    assert all(v.grad is None or float(v.grad.abs().max()) == 0 for k, v in P.items()), [k for k, v in P.items() if v.grad is not None]
    for v in Pp.values():
        v.grad = None
    rgb.sum().backward()
    assert float(P["hash.table"].grad.abs().max()) > 0 and float(P["hash.color.4.weight"].grad.abs().max()) > 0
    assert all(v.grad is None or float(v.grad.abs().max()) == 0 for v in Pp.values())


def test_a_proposal_field_learns():
    """20 Adam steps on the proposal field alone lower the mean proposal loss on the sphere scene"""
    sc = scene()
    Pp = _leaves(sc["Pp"])
    P = {k: v.to(DEV) for k, v in sc["P"].items()}
    opt = torch.optim.Adam([v for k, v in Pp.items() if k != "aabb"], lr=1e-2)
    losses = []
    for _ in range(21):
        loss = _render(sc, Pp, P)[7].mean()
        losses.append(float(loss.detach()))
        opt.zero_grad()
        loss.backward()
        opt.step()
    print("mean proposal loss over 20 Adam steps: %.4e -> %.4e" % (losses[0], losses[-1]))
    assert all(math.isfinite(x) for x in losses) and losses[0] > 0 and losses[-1] < losses[0]


def test_the_four_calls_are_capturable():
    """weights forward + adjoint and the proposal loss forward + adjoint in one torch.cuda.graph: a linear capture on one stream; the replay
    gives the eager bits, and again after the density changed in place"""
    case = PR.make_case(65, seed=765)
    e, f = _rays(case["e"]), _rays(case["f"])
    d = dev(case["dir"])
    gen = torch.Generator().manual_seed(2)
    dens = (torch.rand(case["e"]["P"], generator=gen) * 40).to(DEV)
    w_f, g_w, g_loss = dev(case["f"]["w"]), torch.randn(case["e"]["P"], generator=gen).to(DEV), torch.randn(65, generator=gen).to(DEV)
    Pe, Pf, R = case["e"]["P"], case["f"]["P"], 65

    def run():
        w, trans = torch.zeros(Pe, device=DEV), torch.zeros(R, device=DEV)
        _lib.call("packed_weights", dens, e.deltas, e.ray_start, e.ray_count, R, Pe, w, trans)
        lo, hi, cdf, g_w_e, g_dens = (torch.zeros(Pe, device=DEV) for _ in range(5))
        span, coef, loss = torch.zeros(Pf, 2, dtype=torch.int32, device=DEV), torch.zeros(Pf, device=DEV), torch.zeros(R, device=DEV)
        _lib.call("packed_envelope", w, e.t, e.deltas, e.ray_start, e.ray_count, d, R, Pe, lo, hi, cdf)
        _lib.call("packed_proposal_forward", lo, hi, cdf, e.ray_start, e.ray_count, Pe, w_f, f.t, f.deltas, f.ray_start, f.ray_count, Pf, d, R, PR.EPS, span, coef, loss)
        _lib.call("packed_proposal_backward", g_loss, span, coef, w, e.ray_start, e.ray_count, Pe, f.ray_start, f.ray_count, Pf, R, g_w_e)
        _lib.call("packed_weights_backward", dens, e.deltas, e.ray_start, e.ray_count, R, Pe, g_w_e + g_w, trans, g_dens)
        return w, lo, cdf, span, coef, loss, g_w_e, g_dens

    side = torch.cuda.Stream()  # the warm-up runs on a side stream; the capture itself is linear
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager0 = [x.clone() for x in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(outs, eager0):
        assert torch.equal(x, y) and bool(torch.isfinite(x.float()).all())
    with torch.no_grad():
        dens.mul_(torch.linspace(1e-4, 1.0, Pe, device=DEV) ** 4)
    graph.replay()
    torch.cuda.synchronize()
    eager1 = [x.clone() for x in run()]
    for x, y in zip(outs, eager1):
        assert torch.equal(x, y)
    assert not torch.equal(eager1[5], eager0[5]) and not torch.equal(eager1[7], eager0[7])  # loss, g_density: it did change
