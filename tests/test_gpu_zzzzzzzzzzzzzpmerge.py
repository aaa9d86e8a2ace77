"""Merge of two packed sample lists on the device (csrc/pmerge.hip through lab4d_amd/packed.py and hashfield.render_packed_pair): the kernels
against the CPU twin (tests/host_harness/pmerge/pmerge_host.cpp) WORD FOR WORD, then the host layer -- the two identities on a marched list,
merge + merge_rows + packed.composite against the float64 compositing of the stable-sorted concatenation, render_packed_pair against
render_packed, graph capture."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occgrid_checks as OC  # noqa: E402
import packed_checks as PC  # noqa: E402
import pmerge_checks as PM  # noqa: E402

from lab4d_amd import _lib, hashfield, mlp, occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIST_KEYS = ("t_a", "deltas_a", "start_a", "count_a", "t_b", "deltas_b", "start_b", "count_b")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_merge(case, d, cap, pad=PM.PAD):
    """the library's two calls around torch's exclusive sum on buffers pre-filled with the sentinels of PM.empty_buffers (cap + pad rows in
    the merged buffers: the rows behind the capacity show that they were left alone) -> the dict of PM.host_merge"""
    R, Pa, Pb = case["R"], case["Pa"], case["Pb"]
    count = torch.full((R,), int(PM.SENTINEL_I), dtype=torch.int32, device=DEV)
    _lib.call("packed_merge_count", d["start_a"], d["count_a"], Pa, d["start_b"], d["count_b"], Pb, R, count)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count
    out = {k: dev(v) for k, v in PM.empty_buffers(case, cap, pad).items()}
    _lib.call("packed_merge_write", d["t_a"], d["deltas_a"], d["start_a"], d["count_a"], Pa, d["t_b"], d["deltas_b"], d["start_b"], d["count_b"], Pb, R, start, cap,
              out["t"], out["deltas"], out["ray_idx"], out["src"], out["pos_a"], out["pos_b"], out["ray_count"], out["total"], out["overflow"])
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(ray_start=start.cpu().numpy(), count=count.cpu().numpy(), total=int(res["total"][0]), overflow=bool(res["overflow"][0]), R=R, cap=cap)
    return res


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1025])
def test_kernels_equal_the_cpu_twin_word_for_word(R):
    """the lists of tests/pmerge_checks.py (lengths 0 / 1 / 2 / 63 / 64 / 65 / 129 / 200 paired, gaps, a (start, count) that leaves [0, P) in
    each list, ties on the lattice k / 64, the identical ray, A behind B) at the capacities total, total - 1, the middle of a ray and 0:
    every output array, total and overflow; the sentinels show the rows behind the capacity that were left alone"""
    lib = PM.build_host()
    case = PM.make_pair(R, seed=300 + R)
    d = {k: dev(case[k]) for k in LIST_KEYS}
    full = PM.host_merge(lib, case)
    caps = PM.capacities(case, full["total"], full["count"], full["ray_start"])
    assert len(caps) == 4
    for cap in caps:
        ref, got = PM.host_merge(lib, case, cap), device_merge(case, d, cap)
        PM.assert_same(got, ref, (R, cap))
        assert (got["src"][cap:] == PM.SENTINEL_I).all() and (got["t"][cap:] == PM.SENTINEL_F).all()


def test_every_wave_runs_several_rays():
    """66,000 short rays: more than the 4 x 16,384 rays that one pass of the largest grid takes, so the first blocks' waves come round again"""
    lib = PM.build_host()
    rng = np.random.default_rng(8)
    R = 66000
    case = {"R": R}
    for w in "ab":
        count = rng.choice(np.int32([0, 1, 2, 3, 70]), R, p=[0.3, 0.3, 0.2, 0.19, 0.01])
        P = int(count.sum())
        case.update({"P" + w: P, "count_" + w: count, "start_" + w: (np.cumsum(count) - count).astype(np.int32), "deltas_" + w: rng.random(P).astype(np.float32)})
        t = (rng.integers(0, 8, P) / 64.0).astype(np.float32)
        for s, n in zip(case["start_" + w], count):
            t[s:s + n].sort()
        case["t_" + w] = t
    ref = PM.host_merge(lib, case)
    got = device_merge(case, {k: dev(case[k]) for k in LIST_KEYS}, ref["cap"])
    assert ref["total"] == case["Pa"] + case["Pb"] > 100000
    PM.assert_same(got, ref, "66000 rays")


@pytest.mark.parametrize("C", [1, 3, 64])
def test_gather_equals_the_twin_forward_and_adjoint(C):
    lib = PM.build_host()
    case = PM.make_pair(65, seed=77)
    Pa, Pb = case["Pa"], case["Pb"]
    rng = np.random.default_rng(C)
    a, b = rng.standard_normal((Pa, C)).astype(np.float32), rng.standard_normal((Pb, C)).astype(np.float32)
    m = PM.host_merge(lib, case, cap=PM.host_merge(lib, case)["total"] - 40, pad=0)
    cap = m["cap"]
    g_out = rng.standard_normal((cap, C)).astype(np.float32)
    odd = np.array([-1, 0, Pa - 1, Pa, Pa + Pb - 1, Pa + Pb, 2 ** 31 - 1, -2 ** 31], np.int32)
    forms = [(a, Pa, b, Pb, m["src"]), (a, Pa, None, Pb, m["src"]), (None, Pa, b, Pb, m["src"]), (a, Pa, b, Pb, odd),
             (g_out, cap, None, 0, m["pos_a"]), (g_out, cap, None, 0, m["pos_b"])]  # (the last two: the adjoint of each part)
    for i, (x, nx, y, ny, idx) in enumerate(forms):
        want = PM.host_gather(lib, x, nx, y, ny, idx, C)
        out = torch.full((idx.shape[0], C), float(PM.SENTINEL_F), device=DEV)
        _lib.call("packed_merge_gather", None if x is None else dev(x), nx, None if y is None else dev(y), ny, dev(idx), idx.shape[0], C, out)
        assert np.array_equal(PM.words(out.cpu().numpy()), PM.words(want)), (C, i)
    assert (m["pos_a"] == -1).any() and (m["pos_b"] == -1).any()


# ---------------------------------------------------------------------------------------------------
# a marched list
# ---------------------------------------------------------------------------------------------------
G, K_MAX, DT = 32, 200, 0.015


def new_grid(aabb, occ):
    grid = occgrid.OccupancyGrid(dev(aabb), G=G)
    grid.bits.copy_(dev(OC.pack(occ).view(np.int32)))
    return grid


@functools.lru_cache(None)
def marched_list():
    """65 rays marched through the sphere grid of tests/occgrid_checks.py; the capacity leaves parked rows behind the total"""
    o, d, tr = PC.outside_rays(65, 21, aabb=OC.AABB)
    tr[:, 0], tr[:, 1] = 0.0, 3.0
    grid = new_grid(OC.AABB, OC.sphere_occupancy(G))
    total = int(packed.march(grid, dev(o), dev(d), dev(tr), DT, 0, k_max=K_MAX).total)
    rays = packed.march(grid, dev(o), dev(d), dev(tr), DT, total + 9, k_max=K_MAX)
    assert int(rays.total) == total > 100 and int(rays.ray_count.max()) > 5
    return rays, total


def test_merging_with_an_empty_list_returns_the_list():
    rays, total = marched_list()
    nothing = types.SimpleNamespace(t=torch.zeros(4, device=DEV), deltas=torch.zeros(4, device=DEV), ray_start=torch.zeros(65, dtype=torch.int32, device=DEV),
                                    ray_count=torch.zeros(65, dtype=torch.int32, device=DEV))
    for a, b in ((rays, nothing), (nothing, rays)):
        m = packed.merge(a, b)
        assert isinstance(m, packed.MergedRays) and m.cap == rays.cap + 4 and m.R == 65 and (m.Pa, m.Pb) == (a.t.shape[0], b.t.shape[0])
        assert int(m.total) == total and not bool(m.overflow) and m.overflow.dtype == torch.bool
        for k in ("t", "deltas", "ray_idx"):
            assert getattr(m, k).dtype == getattr(rays, k).dtype and torch.equal(getattr(m, k)[:rays.cap].view(torch.int32), getattr(rays, k).view(torch.int32)), k
        assert torch.equal(m.ray_start, rays.ray_start) and torch.equal(m.ray_count, rays.ray_count)
        assert torch.equal(m.from_b[:total], torch.full((total,), a is nothing, device=DEV)) and not bool(m.from_b[total:].any())
        assert bool((m.src[total:] == -1).all()) and bool(((m.pos_b if a is rays else m.pos_a) == -1).all())


def test_splitting_into_even_and_odd_rows_and_merging_gives_back_the_list():
    """the list's rows, strictly ascending in t within a ray, go alternately to two lists; the merge restores the list, and packed.composite
    of the regathered density / colour equals the composite of the original bit for bit"""
    rays, total = marched_list()
    count = rays.ray_count.cpu().numpy()
    place = np.concatenate([np.arange(n) for n in count]) if total else np.zeros(0, np.int64)
    halves = []
    for odd in (0, 1):
        rows = np.flatnonzero(place % 2 == odd)
        n = (count + 1 - odd) // 2
        halves.append((rows, types.SimpleNamespace(t=rays.t[dev(rows)], deltas=rays.deltas[dev(rows)], ray_start=dev((np.cumsum(n) - n).astype(np.int32)),
                                                   ray_count=dev(n.astype(np.int32)))))
    (rows_a, A), (rows_b, B) = halves
    m = packed.merge(A, B)
    assert m.cap == total == int(m.total) and torch.equal(m.ray_start, rays.ray_start) and torch.equal(m.ray_count, rays.ray_count)
    for k in ("t", "deltas", "ray_idx"):
        assert torch.equal(getattr(m, k).view(torch.int32), getattr(rays, k)[:total].view(torch.int32)), k
    every = np.arange(total)  # row j of the list is A's or B's row number (the rank of j among that half's rows)
    assert np.array_equal(m.src.cpu().numpy(), np.where(place % 2 == 0, np.searchsorted(rows_a, every), len(rows_a) + np.searchsorted(rows_b, every)))
    g = torch.Generator().manual_seed(5)
    dens, rgb = (torch.rand(rays.cap, 1, generator=g) * 40).to(DEV), torch.rand(rays.cap, 3, generator=g).to(DEV)
    want, want_mask = packed.composite(dens, rays.deltas, {"rgb": rgb, "depth": rays.t[:, None]}, rays)
    got, got_mask = packed.composite(packed.merge_rows(m, dens[dev(rows_a)], dens[dev(rows_b)]), m.deltas,
                                     {"rgb": packed.merge_rows(m, rgb[dev(rows_a)], rgb[dev(rows_b)]), "depth": m.t[:, None]}, m)
    assert float(want_mask.max()) > 0.5
    assert torch.equal(got_mask, want_mask) and torch.equal(got["rgb"], want["rgb"]) and torch.equal(got["depth"], want["depth"])


def test_composite_through_the_merge_against_float64():
    """random per-row density / colour on both lists of tests/pmerge_checks.py; merge + merge_rows + packed.composite against
    packed_checks.ref_composite on the per-ray stable-sorted concatenation (numpy's argsort, not the kernels' order), forward and the
    gradients of both lists' density and colour, at the project's fp32 bar: the merge adds copies only, so the composite's own bar holds"""
    case = PM.make_pair(65, seed=31)
    Pa, Pb, R = case["Pa"], case["Pb"], 65
    ref_m = PM.ref_merge(case, pad=0)
    total, src = ref_m["total"], ref_m["src"]
    rng = np.random.default_rng(2)
    # tau = density * delta averages 0.026 (deltas 0.5 .. 3): the longest ray, 329 rows, ends at a transmittance of about e^-9
    val = {"dens_a": rng.random((Pa, 1)) * 0.03, "dens_b": rng.random((Pb, 1)) * 0.03, "rgb_a": rng.random((Pa, 3)), "rgb_b": rng.random((Pb, 3))}
    val = {k: v.astype(np.float32) for k, v in val.items()}
    g_mask, g_out = rng.standard_normal(R).astype(np.float32), rng.standard_normal((R, 3)).astype(np.float32)
    ref = PC.ref_composite({"density": np.concatenate([val["dens_a"], val["dens_b"]])[src, 0], "deltas": ref_m["deltas"],
                            "fields": [np.concatenate([val["rgb_a"], val["rgb_b"]])[src]], "modes": [0], "start": ref_m["ray_start"], "count": ref_m["count"],
                            "P": total, "R": R, "g_mask": g_mask, "g_out": g_out})
    want = {}
    for k, g in (("dens", ref["g_density"][:, None]), ("rgb", ref["g_fields"][0])):  # the reference's gradients, back through the numpy order
        both = np.zeros((Pa + Pb, g.shape[1]))
        both[src] = g
        want[k + "_a"], want[k + "_b"] = both[:Pa], both[Pa:]
    A = types.SimpleNamespace(t=dev(case["t_a"]), deltas=dev(case["deltas_a"]), ray_start=dev(case["start_a"]), ray_count=dev(case["count_a"]))
    B = types.SimpleNamespace(t=dev(case["t_b"]), deltas=dev(case["deltas_b"]), ray_start=dev(case["start_b"]), ray_count=dev(case["count_b"]))
    x = {k: dev(v).requires_grad_(True) for k, v in val.items()}
    m = packed.merge(A, B)
    assert m.cap == Pa + Pb and int(m.total) == total
    rendered, mask = packed.composite(packed.merge_rows(m, x["dens_a"], x["dens_b"]), m.deltas, {"rgb": packed.merge_rows(m, x["rgb_a"], x["rgb_b"])}, m)
    ((mask[:, 0] * dev(g_mask)).sum() + (rendered["rgb"] * dev(g_out)).sum()).backward()
    errs = {"mask": PC.rel_max(mask[:, 0].detach().cpu().numpy(), ref["mask"]), "rgb": PC.rel_max(rendered["rgb"].detach().cpu().numpy(), ref["out"])}
    errs.update({"g_" + k: PC.rel_max(x[k].grad.cpu().numpy(), want[k]) for k in val})
    print("composite through the merge:", {k: "%.2e" % v for k, v in errs.items()})
    assert float(ref["mask"].max()) > 0.9 and all(np.abs(w).max() > 0 for w in want.values())
    for k, e in errs.items():
        assert e < PC.FP32_BAR, (k, e)
    assert all(bool(torch.isfinite(x[k].grad).all()) for k in val)


# ---------------------------------------------------------------------------------------------------
# two hash fields
# ---------------------------------------------------------------------------------------------------
R_PAIR = 256


@functools.lru_cache(None)
def pair_fixture():
    """Two small hash fields (log2_T 12, n_max 128) from make_weights: `a` in a box of three quarters of the edge inside `b`'s box, in the
    same frame; 256 rays aimed at the large box, both fields behind a sphere grid of their own box; every ray parameter in the same units."""
    cfg = {"L": 16, "F": 2, "log2_T": 12, "n_min": 16, "n_max": 128}
    Pa, cfg_a = hashfield.make_weights(3, cfg)
    Pb, cfg_b = hashfield.make_weights(4, cfg)
    Pa["aabb"] = Pb["aabb"] * 0.75
    for P in (Pa, Pb):
        P["hash.table"] = P["hash.table"] * 1e3
    o, d, tr = PC.outside_rays(R_PAIR, 21, aabb=Pb["aabb"].numpy())
    tr[:, 0], tr[:, 1] = 0.0, 3.0
    occ = OC.sphere_occupancy(G)
    out = {"cfg": (cfg_a, cfg_b), "P": (Pa, Pb), "o": dev(o), "d": dev(d), "tr": dev(tr), "occ": occ}
    out["cap"] = tuple(int(packed.march(new_grid(P["aabb"].numpy(), occ), out["o"], out["d"], out["tr"], DT, 0, k_max=K_MAX).total) + 64 for P in (Pa, Pb))
    assert out["cap"][0] > 64 + 100 and out["cap"][1] > 64 + 1000, out["cap"]
    return out


def pair_fields(fx, requires_grad=False, empty_b=False):
    fields = []
    for i in (0, 1):
        P = {k: (v.to(DEV).clone().requires_grad_(requires_grad and k != "aabb")) for k, v in fx["P"][i].items()}
        grid = new_grid(fx["P"][i]["aabb"].numpy(), fx["occ"])
        if i == 1 and empty_b:
            grid.bits.zero_()
        fields.append(hashfield.PackedField(P, fx["cfg"][i], grid, fx["o"], fx["d"], fx["tr"], DT, fx["cap"][i]))
    return fields


def test_render_packed_pair_with_an_empty_second_field_is_render_packed():
    """b's grid emptied: rgb, mask and depth equal render_packed(a) bit for bit and mask_b == 0.  mask_a is the rendered density_a over
    (itself + 0 + 1e-6), the rule of utils/render_utils.py:172-183 -- with D = packed.composite's rendering of a's own density on a's own
    list, D / (D + 1e-6) bit for bit.  (The issue words this check as mask / (mask + 1e-6); the rendered density_a is the weighted mean of
    the density, not the mask, so the check is held against the rendering it is defined by.)"""
    fx = pair_fixture()
    with torch.no_grad():
        a, b = pair_fields(fx, empty_b=True)
        out = hashfield.render_packed_pair(a, b, prec=mlp.PREC_F32, k_max=K_MAX)
        rgb, mask, depth, total, ovf = hashfield.render_packed(a.P, a.cfg, a.grid, a.origin, a.dir, a.t_range, a.dt, a.cap, prec=mlp.PREC_F32, k_max=K_MAX)
        rays = packed.march(a.grid, a.origin, a.dir, a.t_range, a.dt, a.cap, k_max=K_MAX)
        dens = hashfield.forward(a.P, a.cfg, rays.xyz, rays.dirs, spf=a.cap, prec=mlp.PREC_F32)[1]
        D = packed.composite(dens, rays.deltas, {"density": dens}, rays)[0]["density"]
    assert isinstance(out, hashfield.PairRender) and tuple(out.mask_a.shape) == tuple(out.mask_b.shape) == (R_PAIR, 1)
    assert torch.equal(out.rgb, rgb) and torch.equal(out.mask, mask) and torch.equal(out.depth, depth) and float(mask.max()) > 0.05
    assert int(out.total_b) == 0 and int(out.total_a) == int(total) == int(out.total) > 100 and not bool(out.overflow | out.overflow_a | out.overflow_b | ovf)
    assert bool((out.mask_b == 0).all()) and torch.equal(out.mask_a, D / (D + 0.0 + 1e-6)) and float(out.mask_a.max()) > 0.99


def test_render_packed_pair_with_both_fields_live():
    fx = pair_fixture()
    a, b = pair_fields(fx, requires_grad=True)
    out = hashfield.render_packed_pair(a, b, prec=mlp.PREC_F32, k_max=K_MAX)
    assert int(out.total) == int(out.total_a) + int(out.total_b) and int(out.total_a) > 100 and int(out.total_b) > 1000
    assert not bool(out.overflow | out.overflow_a | out.overflow_b)
    for k in ("rgb", "mask", "depth", "mask_a", "mask_b"):
        assert bool(torch.isfinite(getattr(out, k)).all()), k
    mask_a, mask_b = out.mask_a.detach(), out.mask_b.detach()
    assert bool((mask_a + mask_b <= 1).all()) and float(mask_a.max()) > 0.05 and float(mask_b.max()) > 0.5
    both = (mask_a > 0.05) & (mask_b > 0.05)
    assert int(both.sum()) > 5  # rays that see both fields
    g = torch.Generator().manual_seed(9)
    w = [torch.randn(R_PAIR, c, generator=g).to(DEV) for c in (3, 1, 1, 1, 1)]
    sum((getattr(out, k) * x).sum() for k, x in zip(("rgb", "mask", "depth", "mask_a", "mask_b"), w)).backward()
    for f in (a, b):
        for k, v in f.P.items():
            if k != "aabb":
                assert v.grad is not None and bool(torch.isfinite(v.grad).all()), k
        assert float(f.P["hash.table"].grad.abs().max()) > 0 and float(f.P["logibeta"].grad.abs().max()) > 0


def test_merge_and_composite_are_capturable():
    """merge + merge_rows + composite in one torch.cuda.graph: a linear capture on one stream, no side streams inside it; the replay gives
    the eager bits, and again after the inputs changed in place"""
    case = PM.make_pair(65, seed=31)
    A = types.SimpleNamespace(t=dev(case["t_a"]), deltas=dev(case["deltas_a"]), ray_start=dev(case["start_a"]), ray_count=dev(case["count_a"]))
    B = types.SimpleNamespace(t=dev(case["t_b"]), deltas=dev(case["deltas_b"]), ray_start=dev(case["start_b"]), ray_count=dev(case["count_b"]))
    g = torch.Generator().manual_seed(1)
    dens = [(torch.rand(n, 1, generator=g) * 0.03).to(DEV) for n in (case["Pa"], case["Pb"])]
    rgb = [torch.rand(n, 3, generator=g).to(DEV) for n in (case["Pa"], case["Pb"])]

    def run():
        with torch.no_grad():
            m = packed.merge(A, B)
            rendered, mask = packed.composite(packed.merge_rows(m, *dens), m.deltas, {"rgb": packed.merge_rows(m, *rgb)}, m)
            return m.src, m.pos_a, m.pos_b, m.ray_count, m.total, rendered["rgb"], mask

    side = torch.cuda.Stream()  # the warm-up runs on a side stream; the capture itself is linear
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager0 = [t.clone() for t in run()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(outs, eager0):
        assert torch.equal(x, y)
    with torch.no_grad():  # B moves behind A on every ray, and A's density changes
        B.t.add_(100.0)
        dens[0].mul_(2.0)
    graph.replay()
    torch.cuda.synchronize()
    eager1 = [t.clone() for t in run()]
    for x, y in zip(outs, eager1):
        assert torch.equal(x, y)
    assert not torch.equal(eager1[0], eager0[0]) and not torch.equal(eager1[5], eager0[5])  # src, rgb: it did change
