"""The hash field's SDF gradient on the device (csrc/hashsdf.hip through lab4d_amd/hashsdf.py and hashfield.py): the kernels against
float64 torch autograd over oracle/hashgrid_oracle.py (tests/hashsdf_checks.py), 1e-4 relative L2 per tensor; against the existing
independent path (forward(get_density=False) and autograd.grad through k_hashgrid_bwd); the adjoint with only some gradients asked for;
eikonal_loss, normals, the special points, render_packed(with_normal=True), graph capture and the argument checks."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hashsdf_checks as HC  # noqa: E402
from test_hashsdf_host import check_specials  # noqa: E402

from lab4d_amd import hashfield, hashsdf, mlp, occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 63, 64, 65, 257, 1025)


def on_device(P, grad=True):
    Pd = {k: v.to(DEV) for k, v in P.items()}
    if grad:
        for k in HC.PARAMS:
            Pd[k].requires_grad_(True)
    return Pd


@functools.lru_cache(None)
def case(name, unit_box=True):
    """field, 1,025 points, cotangents and the float64 truth of every prefix size -- computed once, shared, never modified"""
    P, cfg = HC.field(name, unit_box=unit_box)
    x, share = HC.points(P, cfg, max(SIZES), seed=21)
    g_sdf, g_grad = HC.cotangents(max(SIZES), 7)
    refs = {S: HC.truth(P, cfg, x[:S], g_sdf[:S], g_grad[:S]) for S in SIZES}
    return P, cfg, x, g_sdf, g_grad, refs


def run(P, cfg, x, g_sdf, g_grad, work_rows=3, params=HC.PARAMS):
    Pd = on_device(P)
    sdf, grad = hashfield.sdf_gradient(Pd, cfg, x.to(DEV), work_rows=work_rows)
    loss = 0.0
    if g_sdf is not None:
        loss = loss + (sdf * g_sdf.to(DEV)).sum()
    if g_grad is not None:
        loss = loss + (grad * g_grad.to(DEV)).sum()
    gs = torch.autograd.grad(loss, [Pd[k] for k in params], allow_unused=True)
    return sdf.detach().cpu(), grad.detach().cpu(), {k: g.cpu() for k, g in zip(params, gs)}


@pytest.mark.parametrize("name", sorted(HC.CONFIGS))
def test_kernels_against_float64(name):
    P, cfg, x, g_sdf, g_grad, refs = case(name)
    worst = {}
    for S in SIZES:
        sdf, grad, got = run(P, cfg, x[:S], g_sdf[:S], g_grad[:S], work_rows=3)
        ref = refs[S]
        errs = {"sdf": HC.rel_l2(sdf, ref["sdf"]), "grad": HC.rel_l2(grad, ref["grad"])}
        for k in HC.PARAMS:
            errs[k] = HC.rel_l2(got[k], ref[k])
        assert not got["hash.geo.2.weight"][1:].any() and not got["hash.geo.2.bias"][1:].any()  # rows 1..15: exact zeros
        print(name, S, {k: "%.2e" % v for k, v in errs.items()})
        assert max(errs.values()) < HC.TOL, (S, errs)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in errs.items()}
    print("worst", name, {k: "%.2e" % v for k, v in worst.items()})
    # the default resident grid gives the same dense gradients up to the order of the sums
    _, _, g3 = run(P, cfg, x, g_sdf, g_grad, work_rows=3)
    _, _, gd = run(P, cfg, x, g_sdf, g_grad, work_rows=None)
    assert all(HC.rel_l2(gd[k], g3[k]) < 1e-5 for k in HC.PARAMS)


@pytest.mark.parametrize("name", sorted(HC.CONFIGS))
def test_against_the_existing_path(name):
    """sdf against forward(get_density=False), grad against autograd.grad of it through k_hashgrid_bwd, at PREC_F32"""
    P, cfg, x, _, _, _ = case(name, unit_box=False)
    Pd = on_device(P, grad=False)
    xd = x.to(DEV)
    sdf, grad = hashfield.sdf_gradient(Pd, cfg, xd)
    xr = xd.clone().requires_grad_(True)
    d = torch.zeros_like(xr)
    d[:, 2] = 1.0
    sdf_old = hashfield.forward(Pd, cfg, xr, d, spf=xr.shape[0], prec=mlp.PREC_F32, get_density=False)[1]
    grad_old, = torch.autograd.grad(sdf_old.sum(), xr)
    e = (HC.rel_l2(sdf.cpu(), sdf_old.detach().cpu()), HC.rel_l2(grad.cpu(), grad_old.cpu()))
    print(name, "sdf %.2e grad %.2e" % e)
    assert max(e) < HC.TOL
    # outside the box the two agree as well
    out = torch.tensor([[0.5, 0.0, 0.0], [0.0, -0.3, 0.05]], device=DEV)
    s_new = hashfield.sdf_gradient(Pd, cfg, out)[0]
    s_old = hashfield.forward(Pd, cfg, out, torch.tensor([[0.0, 0.0, 1.0]] * 2, device=DEV), spf=2, prec=mlp.PREC_F32, get_density=False)[1]
    assert HC.rel_l2(s_new.cpu(), s_old.cpu()) < HC.TOL


def test_partial_gradients_equal_the_full_call():
    P, cfg, x, g_sdf, g_grad, _ = case("a")
    S = 257
    x, g_sdf, g_grad = x[:S], g_sdf[:S], g_grad[:S]
    _, _, full = run(P, cfg, x, g_sdf, g_grad)
    _, _, tab = run(P, cfg, x, g_sdf, g_grad, params=("hash.table",))
    assert HC.rel_l2(tab["hash.table"], full["hash.table"]) < 1e-6  # (atomics: the order of arrival differs)
    _, _, lin = run(P, cfg, x, g_sdf, g_grad, params=HC.PARAMS[1:])
    assert all(torch.equal(lin[k], full[k]) for k in HC.PARAMS[1:])  # the same partial rows in the same order
    _, _, one = run(P, cfg, x, g_sdf, g_grad, params=("hash.geo.0.bias",))
    assert torch.equal(one["hash.geo.0.bias"], full["hash.geo.0.bias"])
    # one cotangent at a time: the two add up to the full call, and each is the truth's
    _, _, only_s = run(P, cfg, x, g_sdf, None)
    _, _, only_g = run(P, cfg, x, None, g_grad)
    ref_s, ref_g = HC.truth(P, cfg, x, g_sdf, None), HC.truth(P, cfg, x, None, g_grad)
    for k in HC.PARAMS:
        assert HC.rel_l2(only_s[k], ref_s[k]) < HC.TOL and HC.rel_l2(only_g[k], ref_g[k]) < HC.TOL, k
        assert HC.rel_l2(only_s[k].double() + only_g[k].double(), full[k]) < 1e-5, k
    assert not only_g["hash.geo.0.bias"].any() and not only_g["hash.geo.2.bias"].any()


@pytest.mark.parametrize("name", sorted(HC.CONFIGS))
def test_eikonal_loss_and_normals(name):
    P, cfg, x, _, _, _ = case(name, unit_box=False)
    S = 1025
    ref = HC.truth(P, cfg, x, eikonal=True)
    Pd = on_device(P)
    loss = hashfield.eikonal_loss(Pd, cfg, x.to(DEV), work_rows=3)
    assert loss.shape == (S, 1)
    gs = torch.autograd.grad(loss.mean(), [Pd[k] for k in HC.PARAMS], allow_unused=True)
    errs = {"loss": HC.rel_l2(loss.detach().cpu(), ref["loss"])}
    for k, g in zip(HC.PARAMS[:4], gs):
        errs[k] = HC.rel_l2(g.cpu(), ref[k])
    assert gs[4] is None or not gs[4].any()
    n = hashfield.normals(Pd, cfg, x.to(DEV))
    errs["normals"] = HC.rel_l2(n.cpu(), torch.nn.functional.normalize(ref["grad"], dim=-1))
    print(name, {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) < HC.TOL, errs
    assert not n.requires_grad and float((n.norm(2, -1) - 1).abs().max()) < 1e-5
    sdf, grad = hashfield.sdf_gradient(Pd, cfg, x.to(DEV))
    assert HC.rel_l2(grad.detach().cpu(), ref["grad"]) < HC.TOL and HC.rel_l2(sdf.detach().cpu(), ref["sdf"]) < HC.TOL


@pytest.mark.parametrize("name", sorted(HC.CONFIGS))
def test_special_points_on_the_device(name):
    P, cfg = HC.field(name)

    def fwd(x):
        s, g, _ = run(P, cfg, x, torch.zeros(x.shape[0], 1), None, params=("hash.geo.2.bias",))
        return s, g

    check_specials(P, cfg, fwd, lambda x, a, b: run(P, cfg, x, a, b)[2])


def test_zero_table_on_the_device():
    P, cfg = HC.field("a", unit_box=False, zero_table=True)
    x, _ = HC.points(P, cfg, 257, seed=5)
    x = torch.cat([x, torch.tensor([[0.5, 0.0, 0.0]])])  # and one point outside the box
    Pd = on_device(P)
    loss = hashfield.eikonal_loss(Pd, cfg, x.to(DEV))
    assert bool((loss.detach()[:-1] == 1).all()) and float(loss.detach()[-1]) == 0.0
    gs = torch.autograd.grad(loss.mean(), [Pd[k] for k in HC.PARAMS], allow_unused=True)
    assert all(g is None or bool(torch.isfinite(g).all()) for g in gs)
    assert not hashfield.normals(Pd, cfg, x.to(DEV)).any()


def test_render_packed_with_normal():
    P, cfg = HC.field("a", unit_box=False)
    Pd = on_device(P, grad=False)
    grid = occgrid.OccupancyGrid(Pd["aabb"], 16)
    g = torch.Generator().manual_seed(3)
    R = 37
    origin = torch.tensor([0.0, 0.0, -0.5]) + 0.05 * torch.randn(R, 3, generator=g)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0]) + 0.15 * torch.randn(R, 3, generator=g), dim=-1)
    t_range = torch.tensor([[0.2, 0.8]]).repeat(R, 1)
    args = (origin.to(DEV), d.to(DEV), t_range.to(DEV), 0.004, 4096)
    base = hashfield.render_packed(Pd, cfg, grid, *args)
    withn = hashfield.render_packed(Pd, cfg, grid, *args, with_normal=True)
    assert len(base) == 5 and len(withn) == 6 and withn[5].shape == (R, 3)
    assert all(torch.equal(a, b) for a, b in zip(base, withn[:5]))
    assert int(base[3]) > R and not bool(base[4])
    rays = packed.march(grid, *args)
    dens = hashfield.forward(Pd, cfg, rays.xyz, rays.dirs, spf=4096)[1]
    want = packed.composite(dens, rays.deltas, {"normal": hashfield.normals(Pd, cfg, rays.xyz)}, rays)[0]["normal"]
    assert torch.equal(withn[5], want) and bool(withn[5].any())


def test_graph_capture():
    """forward + backward captured in one torch.cuda.graph, the table changed between replays, the replay against eager.  The capture
    follows torch's rule for autograd work, as bench.py does: warm-up on a side stream, and NO autograd graph of an eager call alive
    across the capture (every eager result is detached) -- a kept eager graph keeps the parameters' AccumulateGrad nodes bound to the
    stream of the eager call, and the engine would order the capture stream against that stream from inside the capture."""
    P, cfg, x, g_sdf, g_grad, _ = case("a")
    S = 257
    xd, gsd, ggd = x[:S].to(DEV), g_sdf[:S].to(DEV), g_grad[:S].to(DEV)
    Pd = on_device(P)
    params = [Pd[k] for k in HC.PARAMS]
    res = hashfield.resolutions(cfg, DEV)  # (a host-to-device copy: made before the capture)
    names = ["sdf", "grad"] + list(HC.PARAMS)

    def step():
        sdf, grad = hashfield.sdf_gradient(Pd, cfg, xd, res=res, work_rows=3)
        gs = torch.autograd.grad((sdf * gsd).sum() + (grad * ggd).sum(), params)
        return [sdf.detach(), grad.detach()] + [g.detach() for g in gs]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager0 = [t.clone() for t in step()]  # (also allocates the work buffer before the capture)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b, k in zip(outs, eager0, names):
        assert HC.rel_l2(a.cpu(), b.cpu()) < 1e-6, k
    with torch.no_grad():
        Pd["hash.table"].mul_(0.5)  # the table changes between replays
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outs]
    eager1 = step()
    for a, b, k in zip(replayed, eager1, names):
        assert HC.rel_l2(a.cpu(), b.cpu()) < 1e-6, k
    assert HC.rel_l2(replayed[1].cpu(), eager0[1].cpu()) > 0.1  # and it did change


def test_argument_errors_arrive_before_any_launch():
    P, cfg = HC.field("a", unit_box=False)
    Pd = on_device(P)
    x = torch.zeros(4, 3, device=DEV)
    with pytest.raises(RuntimeError, match="must not require grad"):
        hashfield.sdf_gradient(Pd, cfg, x.clone().requires_grad_(True))
    res = hashfield.resolutions(cfg, DEV)
    net = (Pd["hash.geo.0.weight"], Pd["hash.geo.0.bias"], Pd["hash.geo.2.weight"][0], Pd["hash.geo.2.bias"][:1])
    with pytest.raises(RuntimeError, match=r"L \* F = 32"):
        hashsdf.sdf_grad01(x, Pd["hash.table"][:8], res[:8], cfg["log2_T"], *net)
    with pytest.raises(RuntimeError, match=r"work_rows = 513"):
        hashsdf.sdf_grad01(x, Pd["hash.table"], res, cfg["log2_T"], *net, work_rows=513)
    from lab4d_amd import _lib
    lib = _lib.lib()
    p = _lib.ptr(x)
    rc = lib.lab4d_hashsdf_backward(p, p, p, 4, 16, 12, 2, p, p, p, p, p, p, None, p, None, None, None, None, 3, _lib.stream())
    assert rc == -1 and "work buffer" in lib.lab4d_last_error().decode()
    rc = lib.lab4d_hashsdf_forward(p, p, p, 4, 16, 30, 2, p, p, p, p, p, p, _lib.stream())
    assert rc == -1 and "log2_T = 30" in lib.lab4d_last_error().decode()
    torch.cuda.synchronize()
