"""Pruning of the packed sample list on the device (csrc/prune.hip through lab4d_amd/packed.py and hashfield.render_packed_pruned): both
kernels against the CPU twin (tests/host_harness/prune/prune_host.cpp) WORD FOR WORD, hashfield.density against forward(), then the host layer --
render_packed_pruned against render_packed, opacity culling against a gather through src_row, argument checks, graph capture."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occgrid_checks as OC  # noqa: E402
import packed_checks as PC  # noqa: E402
import prune_checks as PR  # noqa: E402

from lab4d_amd import _lib, hashfield, mlp, occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ARRAYS = ("t", "deltas", "xyz", "dirs")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def words(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a).view(np.uint32)


def device_list(case):
    return {k: dev(case[k]) for k in ("density", "deltas", "start", "count") + ARRAYS}


def device_prune(case, d, tau_stop, tau_min, cap):
    """the library's two calls around torch's exclusive sum, with raw thresholds (tau_stop = 0 has no early_stop_eps); keep starts at 7, so
    that the rows of no ray show that they were left alone -> (keep, the dict of PR.host_prune)"""
    R, P = case["R"], case["P"]
    keep = torch.full((P,), 7, dtype=torch.uint8, device=DEV)
    count = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    _lib.call("packed_prune_count", d["density"], d["deltas"], d["start"], d["count"], R, P, tau_stop, tau_min, keep, count)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count
    out = {"t": torch.full((cap,), math.nan, device=DEV), "deltas": torch.full((cap,), math.nan, device=DEV), "xyz": torch.full((cap, 3), math.nan, device=DEV),
           "dirs": torch.full((cap, 3), math.nan, device=DEV), "ray_idx": torch.full((cap,), -7, dtype=torch.int32, device=DEV),
           "src_row": torch.full((cap,), -7, dtype=torch.int32, device=DEV), "ray_count": torch.full((R,), -7, dtype=torch.int32, device=DEV)}
    total, ovf = torch.full((1,), -7, dtype=torch.int32, device=DEV), torch.full((1,), 7, dtype=torch.uint8, device=DEV)
    _lib.call("packed_prune_write", keep, d["start"], d["count"], start, R, P, cap, dev(PR.AABB), d["t"], d["deltas"], d["xyz"], d["dirs"], out["t"],
              out["deltas"], out["xyz"], out["dirs"], out["ray_idx"], out["src_row"], out["ray_count"], total, ovf)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(ray_start=start.cpu().numpy(), count=count.cpu().numpy(), total=int(total), overflow=bool(ovf))
    return keep.cpu().numpy(), res


def assert_equals_twin(got, ref, what):
    assert got["total"] == ref["total"] and got["overflow"] == ref["overflow"], what
    for k in ("count", "ray_start", "ray_count", "ray_idx", "src_row"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k)
    for k in ARRAYS:
        assert got[k].shape == ref[k].shape and np.array_equal(words(got[k]), words(ref[k])), (what, k, int((words(got[k]) != words(ref[k])).sum()))


THRESHOLDS = [PR.thresholds(e, a) for e in PR.EPS for a in PR.ALPHA] + [(math.inf, 0.0), (0.0, 0.0)]  # (both rules off; every row behind a positive prefix drops)


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1025])
def test_kernels_equal_the_cpu_twin_word_for_word(R):
    """the lists of tests/prune_checks.py (lengths 0 / 1 / 2 / 63 / 64 / 65 / 129 / 200, gaps, a (start, count) that leaves [0, P)) at the six
    threshold pairs, both rules off and tau_stop = 0, each at the capacities total, total - 1 and 0: every output array, keep (7 = never
    written in the rows of no ray), total and overflow"""
    lib = PR.build_host()
    case = PR.make_list(R, seed=100 + R)
    d = device_list(case)
    kept = []
    for tau_stop, tau_min in THRESHOLDS:
        keep_ref, _ = PR.host_count(lib, case, tau_stop, tau_min)
        total = PR.host_prune(lib, case, tau_stop, tau_min)["total"]
        for cap in sorted({total, max(total - 1, 0), 0}):
            ref = PR.host_prune(lib, case, tau_stop, tau_min, cap=cap)
            keep, got = device_prune(case, d, tau_stop, tau_min, cap)
            assert np.array_equal(keep, keep_ref), (R, tau_stop, tau_min, cap, "keep")
            assert_equals_twin(got, ref, (R, tau_stop, tau_min, cap))
        kept.append(total)
    owned = sum(PR.rows_of(case, r)[1] for r in range(R))
    assert kept[6] == owned and (R < 63 or 0 < kept[7] < kept[3] < kept[0] < owned)  # (both off; tau_stop = 0; eps 1e-2; eps 1e-4)


def test_every_wave_runs_several_rays():
    """66,000 short rays: more than the 4 x 16,384 rays that one pass of the largest grid takes, so the first blocks' waves come round again"""
    lib = PR.build_host()
    rng = np.random.default_rng(8)
    R = 66000
    count = rng.choice(np.int32([0, 1, 2, 3, 70]), R, p=[0.3, 0.3, 0.2, 0.19, 0.01])
    start = (np.cumsum(count) - count).astype(np.int32)
    P = int(count.sum())
    case = {"R": R, "P": P, "start": start, "count": count, "density": (rng.random(P) * 200).astype(np.float32), "deltas": np.full(P, 1 / 64, np.float32),
            "t": rng.random(P).astype(np.float32), "xyz": rng.standard_normal((P, 3)).astype(np.float32), "dirs": rng.standard_normal((P, 3)).astype(np.float32)}
    tau_stop, tau_min = PR.thresholds(1e-2, 0.05)
    ref = PR.host_prune(lib, case, tau_stop, tau_min, cap=P)
    keep, got = device_prune(case, device_list(case), tau_stop, tau_min, P)
    assert np.array_equal(keep, ref["keep"]) and 0 < ref["total"] < P
    assert_equals_twin(got, ref, "66000 rays")


def rays_of(case, d):
    P, R = case["P"], case["R"]
    return packed.PackedRays(t=d["t"], deltas=d["deltas"], xyz=d["xyz"], dirs=d["dirs"], ray_idx=torch.zeros(P, dtype=torch.int32, device=DEV),
                             ray_start=d["start"], ray_count=d["count"], total=torch.zeros(1, dtype=torch.int32, device=DEV),
                             overflow=torch.zeros(1, dtype=torch.bool, device=DEV), R=R, cap=P)


def test_prune_through_the_python_layer_and_its_argument_checks():
    lib = PR.build_host()
    case = PR.make_list(65, seed=42)
    d = device_list(case)
    rays, aabb = rays_of(case, d), dev(PR.AABB)
    for eps, alpha in ((1e-4, 0.0), (1e-2, 0.05), (0.0, 0.0)):
        ref = PR.host_prune(lib, case, *PR.thresholds(eps, alpha), cap=case["P"])
        got = packed.prune(rays, d["density"][:, None], early_stop_eps=eps, alpha_thre=alpha, aabb=aabb)
        assert isinstance(got, packed.PackedRays) and got.cap == case["P"] and got.R == 65 and got.overflow.dtype == torch.bool and got.src_row.dtype == torch.int32
        res = {k: getattr(got, k).cpu().numpy() for k in ARRAYS + ("ray_start", "ray_count", "ray_idx", "src_row")}
        res.update(total=int(got.total), overflow=bool(got.overflow), count=ref["count"])
        assert_equals_twin(res, ref, (eps, alpha))
    assert not hasattr(rays, "src_row")  # march's objects are unchanged
    # the Python layer's checks
    for kw, word in (({"early_stop_eps": 1.0}, "early_stop_eps"), ({"early_stop_eps": -1e-3}, "early_stop_eps"), ({"alpha_thre": 1.0}, "alpha_thre"),
                     ({"alpha_thre": float("nan")}, "alpha_thre"), ({"cap": -1}, "cap"), ({"cap": 1 << 31}, "cap")):
        with pytest.raises(RuntimeError, match=word):
            packed.prune(rays, d["density"], aabb=aabb, **kw)
    with pytest.raises(RuntimeError, match="density"):
        packed.prune(rays, d["density"][:-1], aabb=aabb)
    with pytest.raises(RuntimeError, match="density"):
        packed.prune(rays, d["density"].double(), aabb=aabb)
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.prune(rays, d["density"].cpu(), aabb=aabb)
    with pytest.raises(RuntimeError, match="aabb"):
        packed.prune(rays, d["density"], aabb=aabb[:5])
    with pytest.raises(TypeError, match="aabb"):
        packed.prune(rays, d["density"])
    # the library's own checks, before any launch: the outputs stay as they were
    L = _lib.lib()
    keep = torch.full((case["P"],), 7, dtype=torch.uint8, device=DEV)
    cnt = torch.full((65,), -7, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    for R, P, tau_stop, tau_min, word in [(65, case["P"], -1.0, 0.0, b"tau_stop"), (65, case["P"], float("nan"), 0.0, b"tau_stop"),
                                          (65, case["P"], 1.0, -1.0, b"tau_min"), (65, case["P"], 1.0, float("inf"), b"tau_min"),
                                          (65, case["P"], 1.0, float("nan"), b"tau_min"), (-1, case["P"], 1.0, 0.0, b"R = -1"), (65, -1, 1.0, 0.0, b"P = -1")]:
        rc = L.lab4d_packed_prune_count(p(d["density"]), p(d["deltas"]), p(d["start"]), p(d["count"]), R, P, tau_stop, tau_min, p(keep), p(cnt), _lib.stream())
        assert rc == -1 and word in L.lab4d_last_error(), (word, L.lab4d_last_error())
    tot, ovf = torch.full((1,), -7, dtype=torch.int32, device=DEV), torch.full((1,), 7, dtype=torch.uint8, device=DEV)
    o = {k: torch.zeros_like(d[k]) for k in ARRAYS}
    idx = torch.zeros(case["P"], dtype=torch.int32, device=DEV)
    for cap, word in ((-1, b"cap"), (1 << 31, b"cap")):
        rc = L.lab4d_packed_prune_write(p(keep), p(d["start"]), p(d["count"]), p(d["start"]), 65, case["P"], cap, p(aabb), p(d["t"]), p(d["deltas"]), p(d["xyz"]),
                                        p(d["dirs"]), p(o["t"]), p(o["deltas"]), p(o["xyz"]), p(o["dirs"]), p(idx), p(idx), p(cnt), p(tot), p(ovf), _lib.stream())
        assert rc == -1 and word in L.lab4d_last_error(), (word, L.lab4d_last_error())
    torch.cuda.synchronize()
    assert bool((keep == 7).all()) and bool((cnt == -7).all()) and int(tot) == -7 and int(ovf) == 7


# ---------------------------------------------------------------------------------------------------
# hash field
# ---------------------------------------------------------------------------------------------------
G, R_RAYS, K_MAX, DT = 32, 257, 200, 0.015  # 3 / 0.015: every candidate up to t1


@functools.lru_cache(None)
def ball_fixture(sdf0=-0.05, table_scale=1e3):
    """A small ball field: the weights and box of tests/test_gpu_zzzzzpacked.py's fixture on a small table (log2_T 12, n_max 128), behind a sphere
    grid; the head's bias is set so that the sdf of the zero encoding is `sdf0`, and 1 / beta = 400: the density is about 400 where the sdf is
    negative, so a ray through the ball (about 0.1 long in the field's frame, tau 0.7 .. 2.9 per row) becomes opaque after a few rows.
    sdf0 = -0.05: the ball is solid.  sdf0 = 0 with a larger table: the sign of the sdf follows the encoding, solid and empty regions alternate
    along a ray (the opacity rule's case)."""
    cfg = {"L": 16, "F": 2, "log2_T": 12, "n_min": 16, "n_max": 128}
    P, cfg = hashfield.make_weights(3, cfg, sdf_bias=0.0)
    P["hash.geo.2.bias"][0] = sdf0 - float(P["hash.geo.2.weight"][0] @ torch.relu(P["hash.geo.0.bias"]))
    P["hash.table"] = P["hash.table"] * table_scale
    P["logibeta"] = torch.tensor([math.log(400.0)])
    aabb = P["aabb"].numpy()
    occ = OC.sphere_occupancy(G)
    o, d, tr = PC.outside_rays(R_RAYS, 21, aabb=aabb)
    tr[:, 0], tr[:, 1] = 0.0, 3.0
    names = [k for k in P if k != "aabb"]
    g = torch.Generator().manual_seed(7)
    cw = [torch.randn(R_RAYS, 3, generator=g).to(DEV), torch.randn(R_RAYS, 1, generator=g).to(DEV), torch.randn(R_RAYS, 1, generator=g).to(DEV)]
    total = PC.host_march(PC.build_host(), o, d, tr, aabb, OC.pack(occ), G, DT, K_MAX)["total"]
    return {"cfg": cfg, "P": P, "aabb": aabb, "occ": occ, "o": o, "d": d, "tr": tr, "names": names, "cw": cw, "total": total, "cap": int(1.25 * total) + 64}


def new_grid(fx):
    grid = occgrid.OccupancyGrid(dev(fx["aabb"]), G=G)
    grid.bits.copy_(dev(OC.pack(fx["occ"]).view(np.int32)))
    return grid


def params(fx):
    return {k: (v.to(DEV).clone().requires_grad_(True) if k in fx["names"] else v.to(DEV)) for k, v in fx["P"].items()}


def loss_of(fx, rgb, mask, depth):
    return (rgb * fx["cw"][0]).sum() + (mask * fx["cw"][1]).sum() + (depth * fx["cw"][2]).sum()


@functools.lru_cache(None)
def full_render():
    """render_packed on the fixture, once: (rgb, mask, depth) and the largest t of the marched list"""
    fx = ball_fixture()
    grid = new_grid(fx)
    o, d, tr = dev(fx["o"]), dev(fx["d"]), dev(fx["tr"])
    with torch.no_grad():
        Pd = {k: v.to(DEV) for k, v in fx["P"].items()}
        rgb, mask, depth, total, ovf = hashfield.render_packed(Pd, fx["cfg"], grid, o, d, tr, DT, fx["cap"], prec=mlp.PREC_F32, k_max=K_MAX)
        t_max = float(packed.march(grid, o, d, tr, DT, fx["cap"], k_max=K_MAX).t.max())
    assert int(total) == fx["total"] and not bool(ovf)
    return rgb, mask, depth, t_max


@pytest.mark.parametrize("prec", [mlp.PREC_F32, mlp.PREC_BF16])
def test_density_equals_forward_bit_for_bit(prec):
    fx = ball_fixture()
    grid = new_grid(fx)
    with torch.no_grad():
        Pd = {k: v.to(DEV) for k, v in fx["P"].items()}
        rays = packed.march(grid, dev(fx["o"]), dev(fx["d"]), dev(fx["tr"]), DT, fx["cap"], k_max=K_MAX)
        want = hashfield.forward(Pd, fx["cfg"], rays.xyz, rays.dirs, spf=fx["cap"], prec=prec)[1]
        got = hashfield.density(Pd, fx["cfg"], rays.xyz, prec)
    assert tuple(got.shape) == (fx["cap"], 1) and got.dtype == want.dtype
    assert torch.equal(got, want) and float(got.max()) > 100 and bool((got[fx["total"]:] == 0).all())  # (the parked rows lie outside the box)


@pytest.mark.parametrize("eps", [1e-2, 1e-4])
def test_render_packed_pruned_against_render_packed(eps):
    """alpha_thre = 0: the surviving rows see the same densities and the same scan, and what is dropped of a ray weighs less than eps in total
    (its transmittance in front of the first dropped row).  With c in [0, 1] and A = sum w c <= M = mask, the pruned colour differs from the full
    one by at most D / (M - D + 1e-6), D <= eps the dropped weight: under 2.1 eps on the rays with M >= 0.5; the issue's bound is 4 eps."""
    fx = ball_fixture()
    rgb_f, mask_f, depth_f, t_max = full_render()
    grid = new_grid(fx)
    Pd = {k: v.to(DEV) for k, v in fx["P"].items()}
    with torch.no_grad():
        out = hashfield.render_packed_pruned(Pd, fx["cfg"], grid, dev(fx["o"]), dev(fx["d"]), dev(fx["tr"]), DT, fx["cap"], prec=mlp.PREC_F32, k_max=K_MAX,
                                             early_stop_eps=eps)
    rgb, mask, depth, total, ovf, kept, kept_ovf = out
    assert int(total) == fx["total"] and not bool(ovf) and not bool(kept_ovf) and kept.dtype == torch.int32 and kept_ovf.dtype == torch.bool
    opaque = mask_f[:, 0] >= 0.5
    errs = {"mask": float((mask - mask_f)[opaque].abs().max()), "rgb": float((rgb - rgb_f)[opaque].abs().max()),
            "depth": float((depth - depth_f)[opaque].abs().max())}
    print("eps %g: %d of %d rays opaque, kept %d of %d rows, t_max %.3f, errors %s" % (eps, int(opaque.sum()), R_RAYS, int(kept), int(total), t_max, errs))
    assert int(opaque.sum()) >= 50
    assert 0 < int(kept) <= int(total)
    if eps == 1e-2:
        assert int(kept) < int(total)
    assert errs["mask"] <= eps + 1e-5, errs
    assert errs["rgb"] <= 4 * eps + 1e-5, errs
    assert errs["depth"] <= (4 * eps + 1e-5) * t_max, errs
    miss = mask_f[:, 0] == 0
    assert int(miss.sum()) > 5 and float(rgb[miss].abs().max()) == 0.0 and float(mask[miss].abs().max()) == 0.0


def test_opacity_culling_equals_a_gather_through_src_row():
    """alpha_thre > 0 drops rows in the middle of a ray: render_packed_pruned against packed.composite on the rows gathered through src_row from an
    un-pruned forward(), values to 1e-5 and the gradients of the table, every Linear and logibeta to the relative-L2 bound of
    tests/test_gpu_zzzzzpacked.py for render_packed (1e-5: the same rows reach the same arithmetic, only the order of the table atomics differs)"""
    fx = ball_fixture(sdf0=0.0, table_scale=3e3)
    grid = new_grid(fx)
    o, d, tr = dev(fx["o"]), dev(fx["d"]), dev(fx["tr"])
    eps, alpha = 1e-4, 0.3
    Pp = params(fx)
    rgb, mask, depth, total, ovf, kept, kept_ovf, normal = hashfield.render_packed_pruned(
        Pp, fx["cfg"], grid, o, d, tr, DT, fx["cap"], prec=mlp.PREC_F32, k_max=K_MAX, early_stop_eps=eps, alpha_thre=alpha, with_normal=True)
    assert tuple(normal.shape) == (R_RAYS, 3) and not bool(kept_ovf)
    gp = dict(zip(fx["names"], torch.autograd.grad(loss_of(fx, rgb, mask, depth), [Pp[k] for k in fx["names"]])))
    # the construction: the field on ALL marched rows, the prune on its density, a gather of colour and density through src_row
    Pg = params(fx)
    rays = packed.march(grid, o, d, tr, DT, fx["cap"], k_max=K_MAX)
    rgb_s, dens_s = hashfield.forward(Pg, fx["cfg"], rays.xyz, rays.dirs, spf=fx["cap"], prec=mlp.PREC_F32)
    pruned = packed.prune(rays, dens_s, early_stop_eps=eps, alpha_thre=alpha, aabb=grid.aabb)
    assert int(pruned.total) == int(kept) and 0 < int(kept) < int(total)
    live = (pruned.src_row >= 0)[:, None].to(torch.float32)
    idx = pruned.src_row.clamp_min(0).long()
    rendered, mask_g = packed.composite(dens_s[idx] * live, pruned.deltas, {"rgb": rgb_s[idx] * live, "depth": pruned.t[:, None]}, pruned)
    gg = dict(zip(fx["names"], torch.autograd.grad(loss_of(fx, rendered["rgb"], mask_g, rendered["depth"]), [Pg[k] for k in fx["names"]])))
    # rows were dropped IN FRONT of a survivor of their ray (by the opacity rule: the stop only drops behind)
    n = int(kept)
    has = pruned.ray_count > 0
    last_src = pruned.src_row[(pruned.ray_start + pruned.ray_count - 1).clamp_min(0).long()]
    culled = int(((last_src - rays.ray_start + 1 - pruned.ray_count) * has).sum())
    assert culled > 10, culled
    errs = {"rgb": float((rgb - rendered["rgb"]).detach().abs().max()), "mask": float((mask - mask_g).detach().abs().max()),
            "depth": float((depth - rendered["depth"]).detach().abs().max())}
    gerrs = {k: float((gp[k] - gg[k]).norm() / gg[k].norm().clamp_min(1e-20)) for k in fx["names"]}
    print("opacity culling: kept %d of %d, %d rows culled in front of a survivor" % (n, int(total), culled), errs, gerrs)
    assert float(mask_g.detach().max()) > 0.5
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)
    for k, e in gerrs.items():
        assert e < 1e-5, (k, e)


def test_pruned_render_is_capturable():
    """march + density + prune + field + composite in one torch.cuda.graph by the rule of DESIGN.md 7f: warm-up on a side stream, and no autograd
    graph of an eager call alive across the capture (the pass runs under no_grad: there is none).  The table changes between replays; the replay
    is held to eager, the prune's layout included.  (The field whose sdf changes sign with the encoding: the negated table moves the surfaces.)"""
    fx = ball_fixture(sdf0=0.0, table_scale=3e3)
    grid = new_grid(fx)
    o, d, tr = dev(fx["o"]), dev(fx["d"]), dev(fx["tr"])
    Pl = {k: v.to(DEV).clone() for k, v in fx["P"].items()}
    res = hashfield.resolutions(fx["cfg"], DEV)

    def run():
        with torch.no_grad():
            rays = packed.march(grid, o, d, tr, DT, fx["cap"], k_max=K_MAX)
            pruned = packed.prune(rays, hashfield.density(Pl, fx["cfg"], rays.xyz, mlp.PREC_F32, res=res), early_stop_eps=1e-2, aabb=grid.aabb)
            return (pruned.ray_count, pruned.src_row) + hashfield.render_packed_pruned(Pl, fx["cfg"], grid, o, d, tr, DT, fx["cap"], prec=mlp.PREC_F32,
                                                                                       k_max=K_MAX, res=res, early_stop_eps=1e-2)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager0 = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        outs = run()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, eager0):
        assert torch.equal(a, b)
    with torch.no_grad():
        Pl["hash.table"].mul_(-1.0)  # another field behind the same grid: other rows survive
    graph.replay()
    torch.cuda.synchronize()
    eager1 = [t.clone() for t in run()]
    for a, b in zip(outs, eager1):
        assert torch.equal(a, b)
    assert not torch.equal(eager1[1], eager0[1]) and not torch.equal(eager1[2], eager0[2])  # src_row, rgb: it did change
    print("capture: kept %d, then %d of %d" % (int(eager0[7]), int(eager1[7]), int(eager1[5])))
