"""Packed ray marching and ragged compositing on the device (csrc/packed.hip through lab4d_amd/packed.py and hashfield.render_packed): the march
kernels against the CPU twin (tests/host_harness/packed_host.cpp) WORD FOR WORD, the compositing kernels against the float64 reference that
tests/test_packed_host.py pins the twin to, then the host layer -- render_packed against the dense lattice through the merged
forward_compacted(occ=grid) path, graph capture, argument checks."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occgrid_checks as OC  # noqa: E402
import packed_checks as PC  # noqa: E402

from lab4d_amd import occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = 0.05


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def new_grid(G, occ=None, aabb=OC.AABB):
    grid = occgrid.OccupancyGrid(dev(aabb), G=G)
    if occ is not None:
        grid.bits.copy_(dev(OC.pack(occ).view(np.int32)))
    return grid


@functools.lru_cache(None)
def ray_set():
    """the special rays of the occupancy tests (1025: the wave and block edges are prefixes of it), with non-finite inputs and t0 > t1 in front"""
    o, d, tr, _ = OC.rays(5)
    o, d, tr = o.copy(), d.copy(), tr.copy()
    o[0, 1], d[1, 2], tr[2, 0], tr[3, 1] = np.nan, np.inf, np.nan, -np.inf
    tr[4] = (2.0, 1.0)
    return o, d, tr


def words(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a).view(np.uint32)


def assert_equals_twin(got, ref, what):
    assert int(got.total) == ref["total"] and bool(got.overflow) == ref["overflow"], what
    assert got.total.dtype == torch.int32 and got.overflow.dtype == torch.bool and got.R == ref["R"] and got.cap == ref["cap"]
    for k in ("ray_count", "ray_start", "ray_idx"):
        assert getattr(got, k).dtype == torch.int32 and np.array_equal(getattr(got, k).cpu().numpy(), ref[k]), (what, k)
    for k in ("t", "deltas", "xyz", "dirs"):
        assert tuple(getattr(got, k).shape) == ref[k].shape, (what, k)
        assert np.array_equal(words(getattr(got, k)), words(ref[k])), (what, k, int((words(getattr(got, k)) != words(ref[k])).sum()))


@pytest.mark.parametrize("G", [5, 32])
def test_march_kernels_equal_the_cpu_twin_word_for_word(G):
    """every R in 1 / 63 / 64 / 65 / 1025 (the wave and block edges of the count pass) with every k_max in 1 / 64 / 65 / 200 and the three
    capacities total, total - 1 and 0, on a random and a sphere grid; then a range that starts far in front of the box"""
    lib = PC.build_host()
    o, d, tr = ray_set()
    n_total = 0
    for occ in (OC.random_occupancy(G, 7, 0.3), OC.sphere_occupancy(G)):
        grid, bits = new_grid(G, occ), OC.pack(occ)
        for R in (1, 63, 64, 65, 1025):
            for k_max in (1, 64, 65, 200):
                total = PC.host_march(lib, o[:R], d[:R], tr[:R], OC.AABB, bits, G, DT, k_max)["total"]
                for cap in sorted({total, max(total - 1, 0), 0}):
                    ref = PC.host_march(lib, o[:R], d[:R], tr[:R], OC.AABB, bits, G, DT, k_max, cap=cap)
                    got = packed.march(grid, dev(o[:R]), dev(d[:R]), dev(tr[:R]), DT, cap, k_max=k_max)
                    assert_equals_twin(got, ref, (G, R, k_max, cap))
                n_total += total
    assert n_total > 5000
    # a far ray range: the first candidate of the span is found from an estimate (t0 = -40: the box is ~800 steps in)
    far = tr.copy()
    far[:, 0] -= 40.0
    ref = PC.host_march(lib, o, d, far, OC.AABB, bits, G, DT, 1000, cap=40000)
    assert 1000 < ref["total"] < 40000
    assert_equals_twin(packed.march(grid, dev(o), dev(d), dev(far), DT, 40000, k_max=1000), ref, "far")


def test_march_on_an_empty_grid_and_without_rays():
    lib = PC.build_host()
    o, d, tr = ray_set()
    G = 5
    empty = np.zeros((G, G, G), bool)
    got = packed.march(new_grid(G, empty), dev(o[:65]), dev(d[:65]), dev(tr[:65]), DT, 7, k_max=64)
    assert_equals_twin(got, PC.host_march(lib, o[:65], d[:65], tr[:65], OC.AABB, OC.pack(empty), G, DT, 64, cap=7), "empty grid")
    assert int(got.total) == 0 and not bool(got.overflow) and bool((got.ray_idx == -1).all()) and bool((got.ray_count == 0).all())
    got = packed.march(new_grid(G), dev(o[:0]), dev(d[:0]), dev(tr[:0]), DT, 7, k_max=64)
    assert_equals_twin(got, PC.host_march(lib, o[:0], d[:0], tr[:0], OC.AABB, OC.pack(np.ones((G, G, G), bool)), G, DT, 64, cap=7), "no rays")


class _Rays:
    def __init__(self, start, count):
        self.ray_start, self.ray_count = dev(start), dev(count)


def device_composite(case, needs=("density", "deltas", "fields")):
    """packed.composite + autograd on the device -> the dict of PC.host_composite (numpy); only the inputs named in `needs` ask for a
    gradient (the others' entries are left out), which decides the branch of the backward kernel"""
    density, deltas = dev(case["density"]).requires_grad_("density" in needs), dev(case["deltas"]).requires_grad_("deltas" in needs)
    fields = {"f%d" % i: dev(f).requires_grad_("fields" in needs) for i, f in enumerate(case["fields"])}
    modes = {"f%d" % i: m for i, m in enumerate(case["modes"])}
    rendered, mask = packed.composite(density, deltas, fields, _Rays(case["start"], case["count"]), modes)
    assert tuple(mask.shape) == (case["R"], 1)
    out = torch.cat([rendered[k].reshape(case["R"], -1) for k in fields], 1)
    loss = (mask[:, 0] * dev(case["g_mask"])).sum() + (out * dev(case["g_out"])).sum()
    res = {"mask": mask[:, 0].detach().cpu().numpy(), "out": out.detach().cpu().numpy()}
    wanted = [("g_density", density), ("g_deltas", deltas)] + [("g_fields", f) for f in fields.values()]
    wanted = [(k, x) for k, x in wanted if x.requires_grad]
    for (k, _), g in zip(wanted, torch.autograd.grad(loss, [x for _, x in wanted])):
        if k == "g_fields":
            res.setdefault(k, []).append(g.cpu().numpy())
        else:
            res[k] = g.cpu().numpy()
    return res


@pytest.mark.parametrize("channels,modes", [((1,), (0,)), ((3,), (0,)), ((4,), (0,)), ((3, 1), (0, 0)), ((3, 4, 1), (0, 1, 2)), ((4, 3, 1), (2, 0, 1)),
                                            ((1, 3, 4), (1, 2, 0))])
def test_composite_kernels_match_float64(channels, modes):
    """the cases of tests/test_packed_host.py: lengths 0, 1, 2, 63, 64, 65, 129 (the last four cross the scan's chunk carry)"""
    case = PC.composite_case(channels, modes, seed=sum(channels) * 10 + len(modes))
    ref = PC.ref_composite(case)
    got = device_composite(case)
    PC.check_composite(got, ref, "kernels %s %s" % (channels, modes))
    assert got["mask"][0] == 0 and (got["out"][0] == 0).all()  # the ray without samples, mode 2 included
    tail = slice(case["P"] - 3, None)  # rows of no ray
    assert (got["g_density"][tail] == 0).all() and all((g[tail] == 0).all() for g in got["g_fields"])
    # and the twin, to the same bar on both sides
    twin = PC.host_composite(PC.build_host(), case["density"], case["deltas"], case["fields"], case["modes"], case["start"], case["count"], case["g_mask"],
                             case["g_out"])
    for k in ("mask", "out", "g_density", "g_deltas"):
        assert PC.rel_max(got[k], twin[k]) < 2 * PC.FP32_BAR, k


@pytest.mark.parametrize("needs", [("fields",), ("deltas",), ("density",), ("deltas", "fields")])
def test_composite_backward_with_some_gradients_absent(needs):
    """The backward kernel's other branches: without g_density the chunk prefixes are parked in g_deltas; without either there is no tau
    gradient and the second pass runs forwards; only one of the two tau gradients.  Each against float64 to the same bar, and equal to the
    word to what the kernel gives when every gradient is asked for (the branches change where a prefix is kept, not the arithmetic)."""
    case = PC.composite_case((3, 4, 1), (0, 1, 2), seed=31)
    ref = PC.ref_composite(case)
    got, full = device_composite(case, needs), device_composite(case)
    assert ("g_density" in got, "g_deltas" in got, "g_fields" in got) == ("density" in needs, "deltas" in needs, "fields" in needs)
    PC.check_composite(got, ref, "kernels, gradients of %s only" % (needs,))
    for k in ("mask", "out", "g_density", "g_deltas"):
        if k in got:
            assert np.array_equal(got[k], full[k]), k
    for a, b in zip(got.get("g_fields", []), full["g_fields"]):
        assert np.array_equal(a, b)


def test_composite_weights_and_transmittance_outputs():
    """the optional per-sample outputs of the C entry point (the Python layer does not ask for them)"""
    from lab4d_amd import _lib
    case = PC.composite_case((3,), (0,), seed=9)
    ref = PC.ref_composite(case)
    density, deltas, f = dev(case["density"]), dev(case["deltas"]), dev(case["fields"][0])
    start, count = dev(case["start"]), dev(case["count"])
    w, T = torch.zeros(case["P"], device=DEV), torch.zeros(case["P"], device=DEV)
    mask, out = torch.empty(case["R"], device=DEV), torch.empty(case["R"], 3, device=DEV)
    fl, _ = packed._field_list([f], [0])
    _lib.call("packed_composite_forward", density, deltas, fl, start, count, case["R"], case["P"], w, T, mask, out)
    assert PC.rel_max(w.cpu().numpy(), ref["weights"]) < PC.FP32_BAR and PC.rel_max(T.cpu().numpy(), ref["transmit"]) < PC.FP32_BAR
    assert PC.rel_max(mask.cpu().numpy(), ref["mask"]) < PC.FP32_BAR


def test_zero_length_ray_between_two_long_ones():
    case = PC.composite_case((3, 1), (0, 2), seed=5, lengths=(129, 0, 70), gap=0)
    solo = PC.composite_case((3, 1), (0, 2), seed=5, lengths=(129, 70), gap=0)  # the same rows without the empty ray
    a = device_composite(case)
    b = device_composite(dict(case, start=solo["start"], count=solo["count"], g_mask=case["g_mask"][[0, 2]], g_out=case["g_out"][[0, 2]], R=2))
    assert a["mask"][1] == 0 and (a["out"][1] == 0).all()
    assert np.array_equal(a["mask"][[0, 2]], b["mask"]) and np.array_equal(a["out"][[0, 2]], b["out"])
    assert np.array_equal(a["g_density"], b["g_density"]) and np.array_equal(a["g_fields"][0], b["g_fields"][0])
    PC.check_composite(a, PC.ref_composite(case), "kernels, empty ray between long ones")


# ---------------------------------------------------------------------------------------------------
# hash field
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def field_fixture():
    """The field of test_gpu_zzhashgrid.py::test_compacted_field_equals_the_full_field (its weights, table scale and box), a sphere grid, and rays
    from outside the box through it."""
    from lab4d_amd import hashfield
    cfg = {"L": 16, "F": 2, "log2_T": 14, "n_min": 16, "n_max": 512}
    P, cfg = hashfield.make_weights(3, cfg, sdf_bias=0.01)
    P["hash.table"] = P["hash.table"] * 3e3
    aabb = P["aabb"].numpy()
    G = 16
    occ = OC.sphere_occupancy(G)
    o, d, tr = PC.outside_rays(200, 21, aabb=aabb)
    tr[:, 0], tr[:, 1] = 0.0, 3.0
    names = [k for k in P if k != "aabb"]
    g = torch.Generator().manual_seed(7)
    R = o.shape[0]
    cw = [torch.randn(R, 3, generator=g).to(DEV), torch.randn(R, 1, generator=g).to(DEV), torch.randn(R, 1, generator=g).to(DEV)]
    dt, k_max = 0.02, 150  # 3 / 0.02: every candidate up to t1
    twin = PC.host_march(PC.build_host(), o, d, tr, aabb, OC.pack(occ), G, dt, k_max)
    return {"cfg": cfg, "P": P, "aabb": aabb, "G": G, "occ": occ, "o": o, "d": d, "tr": tr, "names": names, "cw": cw, "dt": dt, "k_max": k_max, "R": R,
            "total": twin["total"], "cap": int(1.5 * twin["total"])}


def params(fx):
    return {k: (v.to(DEV).clone().requires_grad_(True) if k in fx["names"] else v.to(DEV)) for k, v in fx["P"].items()}


def loss_of(fx, rgb, mask, depth):
    return (rgb * fx["cw"][0]).sum() + (mask * fx["cw"][1]).sum() + (depth * fx["cw"][2]).sum()


def test_render_packed_equals_the_dense_lattice_through_the_merged_path():
    """hashfield.render_packed against ALL K candidates of every ray through forward_compacted(occ=grid) and the dense render_utils.compute_weights
    with delta = dt |d|: a skipped sample has tau = 0 and changes neither w nor T, so the two renderings are the same sums."""
    from lab4d_amd import hashfield, mlp
    from lab4d_amd import render_utils as RU
    fx = field_fixture()
    grid = new_grid(fx["G"], fx["occ"], aabb=fx["aabb"])
    o, d, tr = dev(fx["o"]), dev(fx["d"]), dev(fx["tr"])
    R, K, dt = fx["R"], fx["k_max"], fx["dt"]
    assert 500 < fx["total"] < R * K / 4
    # packed
    Pp = params(fx)
    rgb, mask, depth, total, ovf = hashfield.render_packed(Pp, fx["cfg"], grid, o, d, tr, dt, fx["cap"], prec=mlp.PREC_F32, k_max=K)
    assert tuple(rgb.shape) == (R, 3) and tuple(mask.shape) == (R, 1) and tuple(depth.shape) == (R, 1)
    assert int(total) == fx["total"] and not bool(ovf)
    gp = dict(zip(fx["names"], torch.autograd.grad(loss_of(fx, rgb, mask, depth), [Pp[k] for k in fx["names"]])))
    # dense: the same lattice, formed as the rule forms it (every product and sum rounded to fp32)
    tk, valid = PC.lattice(fx["tr"], dt, K)
    assert valid.all()
    tk = dev(tk)
    xyz = (o[:, None, :] + tk[:, :, None] * d[:, None, :]).reshape(-1, 3)
    ln = d.norm(dim=-1, keepdim=True)
    dirs = (d / ln)[:, None, :].expand(R, K, 3).reshape(-1, 3).contiguous()
    Pd = params(fx)
    rgb_s, dens_s, count, ovf_d = hashfield.forward_compacted(Pd, fx["cfg"], xyz, dirs, fx["cap"], prec=mlp.PREC_F32, occ=grid)
    assert int(count) == fx["total"] and not bool(ovf_d)  # the same samples are kept
    deltas = (dt * ln).expand(R, K).contiguous()
    w, _ = RU.compute_weights(dens_s.reshape(1, R, K, 1), deltas.reshape(1, R, K, 1))
    w = w.reshape(R, K)
    mask_d = w.sum(-1, keepdim=True)
    wn = w / (mask_d + 1e-6)
    rgb_d = (wn[:, :, None] * rgb_s.reshape(R, K, 3)).sum(1)
    depth_d = (wn * tk).sum(1, keepdim=True)
    gd = dict(zip(fx["names"], torch.autograd.grad(loss_of(fx, rgb_d, mask_d, depth_d), [Pd[k] for k in fx["names"]])))
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))
    errs = {"rgb": rel(rgb.detach(), rgb_d.detach()), "mask": rel(mask.detach(), mask_d.detach()), "depth": rel(depth.detach(), depth_d.detach())}
    gerrs = {k: float((gp[k] - gd[k]).norm() / gd[k].norm().clamp_min(1e-20)) for k in fx["names"]}
    print("render_packed against the dense lattice:", errs, gerrs)
    assert float(mask_d.detach().max()) > 0.1 and int((mask_d == 0).sum()) > 5  # opaque rays and rays that miss the ball
    for k, e in errs.items():
        assert e < 1e-4, (k, e)
    # the bound of test_gpu_zzhashgrid.py::test_compacted_field_equals_the_full_field at f32 for two orders of the same table atomics
    # (relative L2 per tensor), here for the table, every Linear and logibeta (measured on an MI355X: 1.5e-7 to 8.8e-7)
    for k, e in gerrs.items():
        assert e < 1e-5, (k, e)
    miss = (mask_d[:, 0] == 0)
    for x in (rgb, mask, depth):
        assert float(x.detach()[miss].abs().max()) == 0.0


def test_march_and_render_packed_are_capturable():
    from lab4d_amd import hashfield, mlp
    fx = field_fixture()
    grid = new_grid(fx["G"], fx["occ"], aabb=fx["aabb"])
    o, d, tr = dev(fx["o"]), dev(fx["d"]), dev(fx["tr"])
    Pl = {k: v.to(DEV) for k, v in fx["P"].items()}
    res = hashfield.resolutions(fx["cfg"], DEV)

    def run():
        with torch.no_grad():
            rays = packed.march(grid, o, d, tr, fx["dt"], fx["cap"], k_max=fx["k_max"])
            return (rays.ray_count, rays.ray_idx) + hashfield.render_packed(Pl, fx["cfg"], grid, o, d, tr, fx["dt"], fx["cap"], prec=mlp.PREC_F32,
                                                                            k_max=fx["k_max"], res=res)

    eager = [t.clone() for t in run()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        outs = run()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert int(outs[5]) == fx["total"] and not bool(outs[6])
    for a, b in zip(outs, eager):
        assert torch.equal(a, b)
    # the grid's bits are read at replay time: a smaller ball, the same graph
    small = OC.sphere_occupancy(fx["G"], r=0.2)
    grid.bits.copy_(dev(OC.pack(small).view(np.int32)))
    graph.replay()
    torch.cuda.synchronize()
    want = [t.clone() for t in run()]
    twin = PC.host_march(PC.build_host(), fx["o"], fx["d"], fx["tr"], fx["aabb"], OC.pack(small), fx["G"], fx["dt"], fx["k_max"])
    assert int(outs[5]) == twin["total"] and 0 < twin["total"] < fx["total"]
    for a, b in zip(outs, want):
        assert torch.equal(a, b)


def test_arguments_are_checked():
    from lab4d_amd import _lib
    grid = new_grid(8)
    o, d, tr = (torch.zeros(4, 3, device=DEV), torch.ones(4, 3, device=DEV), torch.tensor([[0.0, 1.0]] * 4, device=DEV))
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="dt"):
            packed.march(grid, o, d, tr, dt, 16)
    with pytest.raises(RuntimeError, match="k_max"):
        packed.march(grid, o, d, tr, 0.1, 16, k_max=0)
    with pytest.raises(RuntimeError, match="31 bits"):
        packed.march(grid, o, d, tr, 0.1, 16, k_max=1 << 29)
    with pytest.raises(RuntimeError, match="cap"):
        packed.march(grid, o, d, tr, 0.1, -1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.march(grid, o.cpu(), d, tr, 0.1, 16)
    with pytest.raises(RuntimeError, match="disagree"):
        packed.march(grid, o, d[:3], tr, 0.1, 16)
    rays = packed.march(grid, o, d, tr, 0.1, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.composite(torch.zeros(16), rays.deltas, {"rgb": torch.zeros(16, 3, device=DEV)}, rays)
    with pytest.raises(RuntimeError, match="modes"):
        packed.composite(torch.zeros(16, device=DEV), rays.deltas, {"rgb": torch.zeros(16, 3, device=DEV)}, rays, modes={"rgb": 3})
    # the library's own checks, before any launch (the Python layer refuses the same arguments first)
    lib = _lib.lib()
    head = (_lib.ptr(o), _lib.ptr(d), _lib.ptr(tr), _lib.ptr(grid.aabb), _lib.ptr(grid.bits))
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    for G, R, dt, k_max, word in [(8, 4, 0.0, 8, b"dt"), (8, 4, float("nan"), 8, b"dt"), (8, 4, 0.1, 0, b"k_max"), (8, 1 << 22, 0.1, 1 << 9, b"31 bits"),
                                  (1, 4, 0.1, 8, b"G = 1 ")]:
        assert lib.lab4d_packed_march_count(*head, G, R, dt, k_max, _lib.ptr(cnt), _lib.stream()) == -1
        assert word in lib.lab4d_last_error(), (word, lib.lab4d_last_error())
    assert int(cnt.abs().sum()) == 0
