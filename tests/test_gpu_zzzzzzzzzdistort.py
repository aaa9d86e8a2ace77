"""The distortion loss of a packed list on the device (csrc/distort.hip through lab4d_amd/packed.py and hashfield.render_packed /
render_packed_pruned): both kernels against the float64 definition (tests/distort_checks.py) and against the CPU twin
(tests/host_harness/distort/distort_host.cpp) within the project's fp32 bar, then the host layer -- each gradient alone, the rows of no ray,
argument checks, the hash field's renderers, graph capture."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distort_checks as DC  # noqa: E402
import test_gpu_zzzzzzzzprune as TP  # noqa: E402  (7g's ball field: ball_fixture, new_grid, params, G, R_RAYS, K_MAX, DT)

from lab4d_amd import _lib, hashfield, mlp, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
INPUTS = ("density", "deltas", "mid", "width")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Rays:
    def __init__(self, case):
        self.ray_start, self.ray_count = dev(case["start"]), dev(case["count"])


def device_distortion(case, which=("g_density", "g_deltas"), column=False):
    """packed.distortion and autograd of sum(g_loss * loss) -> numpy: loss (R,) and the gradients named in `which` (P,)"""
    x = {k: dev(case[k]) for k in INPUTS}
    if column:
        x = {k: v[:, None] for k, v in x.items()}
    for k in which:
        x[k[2:]].requires_grad_(True)
    loss = packed.distortion(x["density"], x["deltas"], x["mid"], x["width"], Rays(case))
    assert tuple(loss.shape) == (case["R"],) and loss.dtype == torch.float32
    out = {"loss": loss.detach().cpu().numpy()}
    if which:
        grads = torch.autograd.grad((loss * dev(case["g_loss"])).sum(), [x[k[2:]] for k in which])
        out.update({k: g.reshape(-1).cpu().numpy() for k, g in zip(which, grads)})
    return out


def check_case(case, what):
    ref = DC.ref_distortion(case)
    got = device_distortion(case)
    DC.check(got, ref, "kernels vs float64, " + what)
    DC.check(got, DC.host_distortion(DC.build_host(), case), "kernels vs twin, " + what)
    return got, ref


def test_kernels_against_float64_and_the_twin_on_the_composite_list():
    """lengths 0 / 1 / 2 / 63 / 64 / 65 / 129 with 3 unowned rows behind; the inputs also as (P, 1) columns"""
    case = DC.composite_list(seed=4)
    got, ref = check_case(case, "composite_case")
    assert got["loss"][0] == 0 and (got["loss"][1:] > 0).all()
    col = device_distortion(case, column=True)
    for k in DC.OUTPUTS:
        assert np.array_equal(col[k], got[k]), k


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1025])
def test_kernels_against_float64_and_the_twin_on_the_ragged_list(R):
    """the lists of tests/prune_checks.py (lengths up to 200, gaps, a (start, count) that leaves [0, P)); R around the four rays of a block,
    and 1025 rays for more than one block.  Measured on an MI355X: see DESIGN.md 7h."""
    got, ref = check_case(DC.ragged_list(R, seed=100 + R), "ragged R = %d" % R)
    assert (got["loss"] >= 0).all() and (R < 63 or (got["loss"] > 0).sum() > R // 2)


def test_every_wave_runs_several_rays():
    """66,000 short rays: more than the 4 x 16,384 rays that one pass of the largest grid takes, so the first blocks' waves come round again"""
    case = DC.short_rays(66000, seed=8)
    got, ref = check_case(case, "66000 rays")
    assert (got["loss"][case["count"] == 0] == 0).all() and (got["loss"][-2000:] > 0).sum() > 1000


def test_each_gradient_alone_and_the_rows_of_no_ray():
    """g_density alone, g_deltas alone and both are the same words; the library's calls on inputs with NaN in the rows of no ray and a
    sentinel in the outputs: the results of the clean list, the sentinel untouched"""
    case = DC.ragged_list(65, seed=12)
    both = device_distortion(case)
    for k in ("g_density", "g_deltas"):
        alone = device_distortion(case, which=(k,))
        assert np.array_equal(alone[k], both[k]) and np.array_equal(alone["loss"], both["loss"]), k
    assert np.array_equal(device_distortion(case, which=())["loss"], both["loss"])
    dirty = DC.poisoned(case)
    d = {k: dev(dirty[k]) for k in INPUTS + ("start", "count", "g_loss")}
    R, P = case["R"], case["P"]
    loss = torch.full((R,), -7.0, device=DEV)
    gd, gl = torch.full((P,), -7.0, device=DEV), torch.full((P,), -7.0, device=DEV)
    head = [d[k] for k in INPUTS + ("start", "count")] + [R, P]
    _lib.call("packed_distortion_forward", *head, loss)
    _lib.call("packed_distortion_backward", *head, d["g_loss"], gd, gl)
    _lib.call("packed_distortion_backward", *head, d["g_loss"], None, None)  # nothing asked for: no launch
    owned = dirty["owned"]
    assert np.array_equal(loss.cpu().numpy(), both["loss"])
    for g, k in ((gd, "g_density"), (gl, "g_deltas")):
        g = g.cpu().numpy()
        assert (g[~owned] == -7.0).all() and np.array_equal(g[owned], both[k][owned]) and (both[k][~owned] == 0).all(), k
    # through the Python layer the rows of no ray come back as zeros, NaN inputs or not
    got = device_distortion(dirty)
    for k in DC.OUTPUTS:
        assert np.array_equal(got[k], both[k]), k


def test_argument_checks_raise_before_any_launch():
    case = DC.ragged_list(65, seed=42)
    x = {k: dev(case[k]) for k in INPUTS}
    rays = Rays(case)
    for k in INPUTS:
        # (a shorter density sets P: then it is deltas that disagrees)
        for bad, word in ((x[k][:-1], "deltas" if k == "density" else k), (x[k].double(), k), (x[k][:, None, None], k)):
            with pytest.raises(RuntimeError, match=r"packed\.distortion: %s must be float32" % word):
                packed.distortion(*[bad if j == k else x[j] for j in INPUTS], rays)
        with pytest.raises(RuntimeError, match="no CPU path"):
            packed.distortion(*[x[j].cpu() if j == k else x[j] for j in INPUTS], rays)
    wrong = Rays(case)
    wrong.ray_count = wrong.ray_count.long()
    with pytest.raises(RuntimeError, match="ray_start / ray_count"):
        packed.distortion(*[x[j] for j in INPUTS], wrong)
    wrong.ray_count = rays.ray_count[:-1]
    with pytest.raises(RuntimeError, match="ray_start / ray_count"):
        packed.distortion(*[x[j] for j in INPUTS], wrong)
    # the library's own checks, before any launch: the outputs stay as they were
    L, p = _lib.lib(), _lib.ptr
    R, P = case["R"], case["P"]
    loss, g = torch.full((R,), -7.0, device=DEV), torch.full((P,), -7.0, device=DEV)
    ptrs = [p(x[k]) for k in INPUTS] + [p(rays.ray_start), p(rays.ray_count)]
    for r, n, word in ((-1, P, b"R = -1"), (R, -1, b"P = -1"), (1 << 31, P, b"R = 2147483648"), (R, 1 << 31, b"P = 2147483648")):
        assert L.lab4d_packed_distortion_forward(*ptrs, r, n, p(loss), _lib.stream()) == -1 and word in L.lab4d_last_error(), L.lab4d_last_error()
        assert L.lab4d_packed_distortion_backward(*ptrs, r, n, p(loss), p(g), p(g), _lib.stream()) == -1 and word in L.lab4d_last_error(), L.lab4d_last_error()
    for i in range(6):
        holed = ptrs[:i] + [None] + ptrs[i + 1:]
        assert L.lab4d_packed_distortion_forward(*holed, R, P, p(loss), _lib.stream()) == -1 and b"null" in L.lab4d_last_error(), i
        assert L.lab4d_packed_distortion_backward(*holed, R, P, p(loss), p(g), None, _lib.stream()) == -1 and b"null" in L.lab4d_last_error(), i
    assert L.lab4d_packed_distortion_forward(*ptrs, R, P, None, _lib.stream()) == -1 and b"loss" in L.lab4d_last_error()
    assert L.lab4d_packed_distortion_backward(*ptrs, R, P, None, p(g), None, _lib.stream()) == -1 and b"g_loss" in L.lab4d_last_error()
    torch.cuda.synchronize()
    assert bool((loss == -7.0).all()) and bool((g == -7.0).all())


# ---------------------------------------------------------------------------------------------------
# hash field
# ---------------------------------------------------------------------------------------------------
def list_case(rays, density, dt):
    """a marched or pruned list with the density of its rows as a case of tests/distort_checks.py, in render_packed's metric units"""
    n = lambda t: t.detach().cpu().numpy()
    return {"R": rays.R, "P": rays.cap, "start": n(rays.ray_start), "count": n(rays.ray_count), "density": n(density).reshape(-1), "deltas": n(rays.deltas),
            "mid": n(rays.t * rays.deltas / dt), "width": n(rays.deltas), "g_loss": np.ones(rays.R, np.float32)}


def test_render_packed_with_distortion():
    """7g's ball field (G = 32, 257 rays, k_max 200, fp32).  The first five outputs are the words of the call without the flag; distortion lies
    within the bar of the float64 definition on the density that forward() returns for rays.xyz; the gradients of distortion.sum() to the table,
    every geometry Linear and logibeta lie within 1e-4 relative L2 of the float64 g_density pushed through autograd of that forward()."""
    fx = TP.ball_fixture()
    grid = TP.new_grid(fx)
    o, d, tr = TP.dev(fx["o"]), TP.dev(fx["d"]), TP.dev(fx["tr"])
    kw = dict(prec=mlp.PREC_F32, k_max=TP.K_MAX)
    Pp = TP.params(fx)
    with torch.no_grad():
        plain = hashfield.render_packed(Pp, fx["cfg"], grid, o, d, tr, TP.DT, fx["cap"], **kw)
    out = hashfield.render_packed(Pp, fx["cfg"], grid, o, d, tr, TP.DT, fx["cap"], with_distortion=True, **kw)
    assert len(plain) == 5 and len(out) == 6
    for a, b in zip(plain, out):
        assert torch.equal(a, b.detach())
    assert tuple(out[5].shape) == (TP.R_RAYS, 1) and out[5].dtype == torch.float32
    names = [k for k in fx["names"] if k.startswith("hash.table") or k.startswith("hash.geo") or k == "logibeta"]
    got = dict(zip(names, torch.autograd.grad(out[5].sum(), [Pp[k] for k in names])))
    dist = out[5].detach()
    # the reference: the float64 definition on forward()'s density of the marched rows, its g_density through autograd of that forward()
    Pr = TP.params(fx)
    rays = packed.march(grid, o, d, tr, TP.DT, fx["cap"], k_max=TP.K_MAX)
    dens = hashfield.forward(Pr, fx["cfg"], rays.xyz, rays.dirs, spf=fx["cap"], prec=mlp.PREC_F32)[1]
    ref = DC.ref_distortion(list_case(rays, dens, TP.DT))
    err = DC.rel_max(dist.detach().cpu().numpy()[:, 0], ref["loss"])
    want = dict(zip(names, torch.autograd.grad(dens, [Pr[k] for k in names], grad_outputs=dev(ref["g_density"].astype(np.float32))[:, None])))
    gerrs = {k: float((got[k] - want[k]).norm() / want[k].norm().clamp_min(1e-20)) for k in names}
    empty = rays.ray_count.cpu().numpy() == 0
    print("render_packed distortion: rel_max %.2e, %d rays with distortion > 0, %d empty, max %.3e; gradients (relative L2) %s"
          % (err, int((dist > 0).sum()), int(empty.sum()), float(dist.max()), {k: "%.2e" % v for k, v in gerrs.items()}))
    assert int((dist > 0).sum()) >= 1 and int(empty.sum()) >= 1 and bool((dist.detach().cpu()[:, 0][torch.from_numpy(empty)] == 0).all())
    assert err < DC.FP32_BAR, err
    assert set(names) >= {"hash.table", "hash.geo.0.weight", "hash.geo.0.bias", "hash.geo.2.weight", "hash.geo.2.bias", "logibeta"}
    for k, e in gerrs.items():
        assert float(want[k].norm()) > 0 and e < 1e-4, (k, e)


def test_render_packed_pruned_with_distortion_and_normal():
    """the tuple's order and shapes with both flags, and the distortion of the PRUNED list's own rows against the float64 definition"""
    fx = TP.ball_fixture()
    grid = TP.new_grid(fx)
    o, d, tr = TP.dev(fx["o"]), TP.dev(fx["d"]), TP.dev(fx["tr"])
    kw = dict(prec=mlp.PREC_F32, k_max=TP.K_MAX, early_stop_eps=1e-2)
    Pd = {k: v.to(DEV) for k, v in fx["P"].items()}
    with torch.no_grad():
        plain = hashfield.render_packed_pruned(Pd, fx["cfg"], grid, o, d, tr, TP.DT, fx["cap"], **kw)
        only = hashfield.render_packed_pruned(Pd, fx["cfg"], grid, o, d, tr, TP.DT, fx["cap"], with_distortion=True, **kw)
        out = hashfield.render_packed_pruned(Pd, fx["cfg"], grid, o, d, tr, TP.DT, fx["cap"], with_distortion=True, with_normal=True, **kw)
        rays = packed.march(grid, o, d, tr, TP.DT, fx["cap"], k_max=TP.K_MAX)
        kept = packed.prune(rays, hashfield.density(Pd, fx["cfg"], rays.xyz, mlp.PREC_F32), early_stop_eps=1e-2, aabb=grid.aabb)
        dens = hashfield.forward(Pd, fx["cfg"], kept.xyz, kept.dirs, spf=fx["cap"], prec=mlp.PREC_F32)[1]
    assert len(plain) == 7 and len(only) == 8 and len(out) == 9
    for a, b, c in zip(plain, only, out):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert tuple(out[7].shape) == (TP.R_RAYS, 3) and tuple(out[8].shape) == (TP.R_RAYS, 1) and torch.equal(out[8], only[7])
    assert 0 < int(out[5]) < int(out[3])  # rows were pruned
    err = DC.rel_max(out[8].cpu().numpy()[:, 0], DC.ref_distortion(list_case(kept, dens, TP.DT))["loss"])
    print("render_packed_pruned distortion: rel_max %.2e, kept %d of %d rows" % (err, int(out[5]), int(out[3])))
    assert err < DC.FP32_BAR and float(out[8].max()) > 0


def test_distortion_is_capturable():
    """packed.distortion forward under no_grad in one torch.cuda.graph by 7g's rule for captured work: warm-up on a side stream, no autograd
    graph alive across the capture; the density changes between replays and the replay is held to eager"""
    case = DC.ragged_list(65, seed=3)
    x = {k: dev(case[k]) for k in INPUTS}
    rays = Rays(case)

    def run():
        with torch.no_grad():
            return packed.distortion(x["density"], x["deltas"], x["mid"], x["width"], rays)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager0 = run().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        out = run()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager0)
    x["density"].mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    eager1 = run()
    assert torch.equal(out, eager1) and not torch.equal(eager1, eager0)
