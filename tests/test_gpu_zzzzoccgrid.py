"""The occupancy grid of the hash field on the device (csrc/occgrid.hip through lab4d_amd/occgrid.py and hashfield.py): the three kernels
against the CPU twin (tests/host_harness/occgrid_host.cpp) BIT FOR BIT on the inputs of tests/test_occgrid_host.py, which pins the twin
against float64; then the host layer -- forward_compacted(occ=...), update_occupancy, ray_depths, graph capture."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occgrid_checks as OC  # noqa: E402

from lab4d_amd import occgrid  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
S_MASK = 64 * 1000 + 1


@functools.lru_cache(None)
def host():
    return OC.build_host()


@functools.lru_cache(None)
def mask_points():
    return OC.mask_points(S_MASK, 17)


@functools.lru_cache(None)
def ray_set():
    return OC.rays(5)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def new_grid(G, occ=None, aabb=OC.AABB, **kw):
    grid = occgrid.OccupancyGrid(dev(aabb), G=G, **kw)
    if occ is not None:
        grid.bits.copy_(dev(OC.pack(occ).view(np.int32)))
    return grid


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("G", [5, 32, 48, 128])
def test_kernels_equal_the_cpu_twin_bit_for_bit(G):
    lib = host()
    # update: a new grid is the twin's new grid; three refreshes (NaN, negative, zero and +inf densities among them)
    grid = new_grid(G, decay=0.95, thresh=0.01)
    ema, bits, n_occ = OC.host_init(lib, G)
    assert np.array_equal(u32(grid.bits), bits) and np.array_equal(u32(grid.ema), ema.view(np.uint32)) and int(grid.n_occupied) == n_occ
    for it in range(3):
        dens = OC.density_volume(G, 100 * G + it)
        n_occ = OC.host_update(lib, dens, ema, bits, G, 0.95, 0.01)
        grid.update(dev(dens) if it else dev(dens).reshape(G, G, G))
        assert np.array_equal(u32(grid.bits), bits), it
        assert np.array_equal(u32(grid.ema), ema.view(np.uint32)), it
        assert int(grid.n_occupied) == n_occ == OC.popcount(bits), it
    assert 0 < n_occ < G ** 3
    # mask
    pts = mask_points()
    for occ in (OC.random_occupancy(G, 3, 0.4), np.ones((G, G, G), bool)):
        got = new_grid(G, occ).mask(dev(pts))
        assert got.dtype == torch.uint8 and got.shape == (S_MASK,)
        ref = OC.host_mask(lib, pts, OC.AABB, OC.pack(occ), G)
        assert np.array_equal(got.cpu().numpy(), ref)
    assert 0 < ref.sum() < S_MASK
    # ray span: t_span as raw words
    o, d, tr, _ = ray_set()
    for occ in (OC.random_occupancy(G, 7), OC.sphere_occupancy(G)):
        span, hit = new_grid(G, occ).ray_span(dev(o), dev(d), dev(tr))
        ref_span, ref_hit, _ = OC.host_ray_span(lib, o, d, tr, OC.AABB, OC.pack(occ), G)
        assert hit.dtype == torch.bool and np.array_equal(hit.cpu().numpy(), ref_hit.astype(bool))
        assert np.array_equal(u32(span), ref_span.view(np.uint32)), int((u32(span) != ref_span.view(np.uint32)).sum())
        assert 0 < ref_hit.sum() < OC.N_RAYS


def test_arguments_are_checked():
    with pytest.raises(RuntimeError, match="G = 1 "):
        occgrid.OccupancyGrid(dev(OC.AABB), G=1)
    with pytest.raises(RuntimeError, match="G = 257 "):
        occgrid.OccupancyGrid(dev(OC.AABB), G=257)
    grid = new_grid(8)
    with pytest.raises(RuntimeError, match="G = 8"):
        grid.update(torch.zeros(9, 9, 9, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        grid.mask(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="disagree"):
        grid.ray_span(torch.zeros(4, 3, device=DEV), torch.zeros(4, 3, device=DEV), torch.zeros(3, 2, device=DEV))
    grid.decay = 1.5
    with pytest.raises(RuntimeError, match="decay"):
        grid.update(torch.zeros(8, 8, 8, device=DEV))
    assert tuple(grid.cell_centers().shape) == (512, 3)
    assert bool(grid.mask(grid.cell_centers()).all())


# ---------------------------------------------------------------------------------------------------
# hash field
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def field_fixture():
    """The fixture and sizes of test_gpu_zzhashgrid.py::test_compacted_field_equals_the_full_field, and its no-grid result (computed once)."""
    from lab4d_amd import hashfield
    cfg = {"L": 16, "F": 2, "log2_T": 14, "n_min": 16, "n_max": 512}
    P, cfg = hashfield.make_weights(3, cfg, sdf_bias=0.01)
    P["hash.table"] = P["hash.table"] * 3e3
    g = torch.Generator().manual_seed(7)
    S = 5000
    xyz = (torch.rand(S, 3, generator=g) * 2 - 1) * 0.2
    dirs = torch.nn.functional.normalize(torch.randn(S, 3, generator=g), dim=-1)
    names = [k for k in P if k != "aabb"]
    cw = [torch.randn(S, 3, generator=g).to(DEV), torch.randn(S, 1, generator=g).to(DEV)]
    fx = {"cfg": cfg, "P": P, "xyz": xyz, "dirs": dirs, "names": names, "cw": cw, "S": S, "cap": 2048}
    fx["base"] = run_field(fx, None)
    return fx


def run_field(fx, occ, weight=None):
    """forward_compacted + the gradients of the test's loss; weight (S,1): the upstream gradients of both outputs are multiplied by it"""
    from lab4d_amd import hashfield, mlp
    P, names = fx["P"], fx["names"]
    Pl = {k: (v.to(DEV).clone().requires_grad_(True) if k in names else v.to(DEV)) for k, v in P.items()}
    rgb, dens, count, ovf = hashfield.forward_compacted(Pl, fx["cfg"], fx["xyz"].to(DEV), fx["dirs"].to(DEV), fx["cap"], prec=mlp.PREC_F32, occ=occ)
    w = 1.0 if weight is None else weight
    gs = torch.autograd.grad((rgb * fx["cw"][0] * w).sum() + (dens * fx["cw"][1] * w).sum() * 1e-2, [Pl[k] for k in names])
    assert not bool(ovf)
    return rgb.detach(), dens.detach(), int(count), dict(zip(names, gs))


def rel_l2(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-20))


def test_fresh_grid_changes_nothing():
    fx = field_fixture()
    r0, d0, c0, g0 = fx["base"]
    r1, d1, c1, g1 = run_field(fx, occgrid.OccupancyGrid(fx["P"]["aabb"].to(DEV), G=128))
    assert torch.equal(r1, r0) and torch.equal(d1, d0) and c1 == c0 and 500 < c0 < 2048
    for k in fx["names"]:
        assert rel_l2(g1[k], g0[k]) < 1e-3, (k, rel_l2(g1[k], g0[k]))  # (two orders of the same atomics)


def test_sphere_grid_masks_outputs_and_gradients():
    fx = field_fixture()
    r0, d0, c0, _ = fx["base"]
    G = 16
    grid = new_grid(G, OC.sphere_occupancy(G), aabb=fx["P"]["aabb"].numpy())
    m = grid.mask(fx["xyz"].to(DEV))
    # the mask is the float64 rule away from the cell faces
    ref, clear = OC.ref_mask(fx["xyz"].numpy(), OC.sphere_occupancy(G), G, aabb=fx["P"]["aabb"].numpy())
    assert np.array_equal(m.cpu().numpy().astype(bool)[clear], ref[clear]) and clear.mean() > 0.99
    r1, d1, c1, g1 = run_field(fx, grid)
    mf = m.to(torch.float32)[:, None]
    assert torch.equal(r1, r0 * mf) and torch.equal(d1, d0 * mf)
    assert float(r1[m == 0].abs().max()) == 0.0 and float(d1[m == 0].abs().max()) == 0.0
    assert c1 == int(m.sum()) and 50 < c1 < c0
    # the gradients are those of the loss with the masked samples' upstream gradients zeroed, on the path without a grid
    _, _, _, gm = run_field(fx, None, weight=mf)
    for k in fx["names"]:
        assert rel_l2(g1[k], gm[k]) < 1e-3, (k, rel_l2(g1[k], gm[k]))
    assert rel_l2(g1["hash.table"], fx["base"][3]["hash.table"]) > 0.1  # (and not those of the unmasked loss)


def ball_field():
    """A hash field whose density is ~10 inside a ball and ~2e-4 away from it: the level-0 table (dense, resolution 16) holds
    20 * (0.3 - |v01 - 0.5|) in feature 0, the geometry net passes relu(feature 0) through, sdf = sdf_bias - relu(...), sdf_bias = 1."""
    from lab4d_amd import hashfield
    cfg = {"L": 16, "F": 2, "log2_T": 14, "n_min": 16, "n_max": 512}
    P, cfg = hashfield.make_weights(0, cfg, sdf_bias=1.0)
    for k in ("hash.table", "hash.geo.0.weight", "hash.geo.0.bias", "hash.geo.2.weight"):
        P[k].zero_()
    P["hash.geo.2.bias"][1:] = 0.0
    n = 17
    ax = torch.arange(n, dtype=torch.float64) / 16 - 0.5
    iz, iy, ix = torch.meshgrid(ax, ax, ax, indexing="ij")  # dense levels index ix + n * (iy + n * iz)
    P["hash.table"][0, :n ** 3, 0] = (20 * (0.3 - torch.sqrt(ix ** 2 + iy ** 2 + iz ** 2))).reshape(-1).float()
    P["hash.geo.0.weight"][0, 0] = 1.0
    P["hash.geo.2.weight"][0, 0] = -1.0
    return P, cfg


def test_update_occupancy_follows_the_density():
    from lab4d_amd import hashfield
    from oracle import hashgrid_oracle as HO
    P, cfg = ball_field()
    G, thresh = 16, 0.01
    Pd = {k: v.to(DEV) for k, v in P.items()}
    grid = occgrid.OccupancyGrid(Pd["aabb"], G=G, thresh=thresh)
    assert hashfield.update_occupancy(Pd, cfg, grid) is grid
    centres = grid.cell_centers()
    P64 = {k: v.double() for k, v in P.items()}
    pts = centres.cpu().double()
    dens = HO.hash_field_forward(P64, cfg, pts, torch.zeros_like(pts))[1][:, 0].numpy()
    lo, hi = int((dens > 2 * thresh).sum()), int((dens > thresh / 2).sum())
    n = int(grid.n_occupied)
    print("update_occupancy: %d cells occupied of %d; float64 density > 2 thresh: %d, > thresh / 2: %d" % (n, G ** 3, lo, hi))
    assert 100 < lo <= n <= hi < G ** 3 / 2
    bits = OC.unpack(u32(grid.bits), G).reshape(-1)
    assert bits[dens > 2 * thresh].all() and not bits[dens < thresh / 2].any() and bits.sum() == n
    assert float(grid.ema.max()) > 5.0 and float(grid.ema.min()) < 1e-3  # ~10 in the ball, ~2e-4 away from it
    # the refreshed grid drops the samples of the empty cells from the field's work
    xyz = (torch.rand(4000, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 0.12
    dirs = torch.nn.functional.normalize(torch.randn(4000, 3, generator=torch.Generator().manual_seed(2)), dim=-1)
    _, d_all, c_all, _ = hashfield.forward_compacted(Pd, cfg, xyz.to(DEV), dirs.to(DEV), 4096)
    _, d_occ, c_occ, _ = hashfield.forward_compacted(Pd, cfg, xyz.to(DEV), dirs.to(DEV), 4096, occ=grid)
    m = grid.mask(xyz.to(DEV))
    assert int(c_all) == 4000 and int(c_occ) == int(m.sum()) and 100 < int(c_occ) < 800  # the occupied cells are ~9 % of the box
    assert torch.equal(d_occ, d_all * m.to(torch.float32)[:, None])


def test_ray_depths_feed_sample_cam_rays():
    from lab4d_amd import render_utils as RU
    M, N, D, G = 2, 96, 16, 16
    g = torch.Generator().manual_seed(4)
    hxy = torch.cat([torch.rand(M, N, 2, generator=g) * 64, torch.ones(M, N, 1)], -1).to(DEV)
    Kinv = torch.tensor([[1 / 200.0, 0, -0.16], [0, 1 / 200.0, -0.16], [0, 0, 1]]).expand(M, 3, 3).contiguous().to(DEV)
    near_far = torch.tensor([[0.1, 1.5], [0.2, 1.2]]).to(DEV)
    aabb = np.array([[-0.12, -0.12, 0.5], [0.12, 0.12, 0.74]], np.float32)  # a box in front of the camera, in the camera's frame
    grid = new_grid(G, OC.sphere_occupancy(G), aabb=aabb)
    dirs = torch.einsum("mij,mnj->mni", Kinv, hxy).contiguous()  # z = 1: the ray parameter is the depth
    origin = torch.zeros_like(dirs)
    depth, hit = grid.ray_depths(origin, dirs, near_far, D)
    assert tuple(depth.shape) == (M, N, D, 1) and tuple(hit.shape) == (M, N) and hit.dtype == torch.bool
    span, hit2 = grid.ray_span(origin.reshape(-1, 3), dirs.reshape(-1, 3), near_far[:, None, :].expand(M, N, 2).reshape(-1, 2).contiguous())
    span, hit2 = span.reshape(M, N, 2), hit2.reshape(M, N)
    assert torch.equal(hit, hit2) and 10 < int(hit.sum()) < M * N - 10
    xyz_cam, _, _, depth_out = RU.sample_cam_rays(hxy, Kinv, near_far, n_depth=D, depth=depth)
    assert torch.equal(depth_out, depth)
    assert torch.allclose(xyz_cam, dirs[:, :, None, :] * depth, rtol=1e-5, atol=1e-7)
    dh, sh = depth[hit][..., 0], span[hit]  # (n_hit, D), (n_hit, 2)
    assert torch.equal(dh[:, 0], sh[:, 0]) and torch.equal(dh[:, -1], sh[:, 1])
    assert bool(((dh >= sh[:, :1]) & (dh <= sh[:, 1:])).all()) and bool((dh[:, 1:] >= dh[:, :-1]).all())
    nf = near_far[:, None, :].expand(M, N, 2)[~hit]
    assert torch.equal(depth[~hit][:, 0, 0], nf[:, 0]) and torch.equal(depth[~hit][:, -1, 0], nf[:, 1])  # no hit: the original range
    # the span covers the ray's occupied cells: every sample of the ORIGINAL range that the float64 rule puts into an occupied cell (clear of the
    # cell faces) lies inside it
    full = RU.sample_cam_rays(hxy, Kinv, near_far, n_depth=256)
    ref, clear = OC.ref_mask(full[0].reshape(-1, 3).cpu().numpy(), OC.sphere_occupancy(G), G, aabb=aabb)
    occupied = torch.from_numpy(ref & clear).reshape(M, N, 256).to(DEV)
    d_full = full[3][..., 0]
    assert int(occupied.sum()) > 300  # (~40 % of the rays cross the ball, a dozen of the 256 samples each)
    assert bool((~occupied | (hit[..., None] & (d_full >= span[..., :1]) & (d_full <= span[..., 1:]))).all())


def test_mask_compact_and_ray_span_are_capturable():
    from lab4d_amd import render_utils as RU
    G = 32
    grid = new_grid(G, OC.sphere_occupancy(G))
    o, d, tr, _ = ray_set()
    pts, o, d, tr = dev(mask_points()), dev(o), dev(d), dev(tr)
    eager = (grid.mask(pts),) + RU.compact(grid.mask(pts)) + grid.ray_span(o, d, tr)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        m = grid.mask(pts)
        idx, count = RU.compact(m)
        span, hit = grid.ray_span(o, d, tr)
    for t in (m, idx, count, span, hit):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    n = int(count)
    assert n == int(eager[2]) and 0 < n < S_MASK
    assert torch.equal(m, eager[0]) and torch.equal(idx[:n], eager[1][:n])
    assert torch.equal(span, eager[3]) and torch.equal(hit, eager[4])
    # the grid's state is read at replay time: after a refresh the same graph sees the new bits
    grid.update(torch.zeros(G, G, G, device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert int(count) == 0 and not bool(hit.any()) and int(grid.n_occupied) == 0
