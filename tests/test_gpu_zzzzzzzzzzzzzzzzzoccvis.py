"""Visibility cull of the occupancy grids on the GPU (csrc/occvis.hip) against the CPU twin of tests/occvis_checks.py, word for word: the mark
kernel across the 64-view LDS tile edge, APPLY, the persistence of a cull through hashfield.update_occupancy(_cascade) with and without
visible_only, the marches of the culling cameras' own rays, graph capture.  tests/test_occvis_host.py pins the twin itself."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conemarch_checks as CC  # noqa: E402
import occgrid_checks as OC  # noqa: E402
import occvis_checks as VC  # noqa: E402

from lab4d_amd import _lib, occgrid, packed  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@functools.lru_cache(None)
def views(base=None):
    groups = VC.camera_groups() if base is None else VC.camera_groups(np.asarray(base, np.float32).reshape(2, 3))
    return groups, VC.all_planes(groups)[1]


@functools.lru_cache(None)
def twin_marks(M, K, G, min_views, first=None):
    """the twin's (words, n_visible) for the first `first` (None: all) of VC.tile_views(M)"""
    planes = VC.tile_views(M)[:first]
    return VC.host_mark(VC.build_host(), planes, CC.cascade_boxes(K), G, min_views)


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("G", [2, 5, 32, 48])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 200])
def test_mark_kernel_equals_the_cpu_twin_word_for_word(M, K, G):
    """min_views = 1, 2, 3 at every M, K and G.  The views are VC.tile_views(M): the ones that see something sit at the first slot, inside
    the first tile, on both sides of every 64-view tile edge and at the end, so that (asserted here) the three min_views
    give three different sets of words, and cutting the list at any tile edge changes the words of every min_views (at G = 32): a kernel that loses a
    later tile, its tail or the count across tiles cannot pass"""
    planes, aabbs = VC.tile_views(M), CC.cascade_boxes(K)
    planes_d, aabbs_d = dev(planes), dev(aabbs)
    wants = {}
    for min_views in (1, 2, 3):
        if min_views > M:
            continue
        want, want_n = wants[min_views] = twin_marks(M, K, G, min_views)
        vis = torch.full((K, OC.n_words(G)), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        n_vis = torch.full((K,), -7, dtype=torch.int32, device=DEV)
        _lib.call("occvis_mark", planes_d, M, aabbs_d, K, G, min_views, vis, n_vis)
        assert np.array_equal(u32(vis), want), (min_views, int((u32(vis) != want).sum()))
        assert n_vis.cpu().tolist() == want_n.tolist(), min_views
    if G >= 32:  # (the coarser grids are all but wholly visible to 200 views)
        assert 0 < wants[1][1].sum() < K * G ** 3
        if M >= 3:
            assert wants[1][1].sum() > wants[2][1].sum() > wants[3][1].sum() > 0
        for edge in range(VC.TILE, M if G == 32 else 0, VC.TILE):  # (a property of the views, shown at one G: 5 is too coarse, 48 only pays the twin again)
            for min_views, (want, _) in wants.items():
                assert not np.array_equal(twin_marks(M, K, G, min_views, first=edge)[0], want), (edge, min_views)


@pytest.mark.parametrize("K,G", [(1, 5), (4, 8), (1, 32), (4, 48)])
def test_apply_equals_the_twin(K, G):
    """bits = old & vis, ema zero exactly on the invisible cells and untouched elsewhere, n_occupied the popcount, the padding bits zero"""
    lib = VC.build_host()
    rng = np.random.default_rng(3 + G)
    occ, vis = rng.random((K, G, G, G)) < 0.5, rng.random((K, G, G, G)) < 0.6
    bits, vbits = CC.pack_levels(occ), CC.pack_levels(vis)
    ema0 = np.stack([OC.density_volume(G, 5 + c) for c in range(K)])
    ema_h, bits_h = ema0.copy(), bits.copy()
    n_h = VC.host_apply(lib, vbits, ema_h, bits_h, G)
    ema_d, bits_d, n_d = dev(ema0), dev(bits.view(np.int32)), torch.full((K,), -7, dtype=torch.int32, device=DEV)
    _lib.call("occvis_apply", dev(vbits.view(np.int32)), ema_d, bits_d, n_d, K, G)
    assert np.array_equal(u32(bits_d), bits_h) and np.array_equal(bits_h, bits & vbits)
    assert np.array_equal(u32(ema_d), ema_h.view(np.uint32))
    v = vis.reshape(K, -1)
    assert (ema_h[~v] == 0).all() and np.array_equal(ema_h[v].view(np.uint32), ema0[v].view(np.uint32))
    assert n_d.cpu().tolist() == n_h.tolist() == [OC.popcount(w) for w in bits_h]
    if G ** 3 % 32:
        assert (u32(bits_d)[:, -1] >> np.uint32(G ** 3 % 32) == 0).all()


# ---------------------------------------------------------------------------------------------------
# persistence through the field's refresh
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def field_fixture():
    """the field of tests/test_gpu_zzzzzzzzzzzzzzzzconemarch.py (its weights, table scale and box; sdf_bias so that a surface exists)"""
    from lab4d_amd import hashfield
    cfg = {"L": 16, "F": 2, "log2_T": 14, "n_min": 16, "n_max": 512}
    P, cfg = hashfield.make_weights(3, cfg, sdf_bias=0.01)
    P["hash.table"] = P["hash.table"] * 3e3
    return {k: v.to(DEV) for k, v in P.items()}, cfg


def median_density(P, cfg, grid):
    from lab4d_amd import hashfield
    with torch.no_grad():
        pts = grid.cell_centers().reshape(-1, 3)
        dirs = torch.zeros_like(pts)
        dirs[:, 2] = 1.0
        return float(hashfield.forward(P, cfg, pts, dirs, spf=pts.shape[0])[1].median())


def test_a_culled_grid_stays_culled_through_the_refresh():
    """G = 32: after cull_invisible, hashfield.update_occupancy gives (the bits of an unculled twin grid after the same update) & visible,
    twice over (the second update runs on a decayed ema); visible_only=True gives the same words, n_occupied and ema on the visible cells,
    and no overflow at a capacity of n_visible rows"""
    from lab4d_amd import hashfield
    P, cfg = field_fixture()
    box = P["aabb"]
    G = 32
    thresh = median_density(P, cfg, occgrid.OccupancyGrid(box, G=G))
    groups, _ = views(tuple(box.cpu().numpy().reshape(-1).tolist()))
    planes = dev(VC.all_planes([groups[1], groups[4], groups[5]])[1])
    plain, culled, lean = (occgrid.OccupancyGrid(box, G=G, thresh=thresh) for _ in range(3))
    assert culled.cull_invisible(planes) is culled and lean.cull_invisible(planes) is lean
    want_vis, want_n = VC.host_mark(VC.build_host(), planes.cpu().numpy(), box.cpu().numpy().reshape(1, 6), G, 1)
    assert np.array_equal(u32(culled.visible), want_vis[0]) and culled.n_visible.cpu().tolist() == want_n.tolist()
    n_vis = int(want_n[0])
    assert 0 < n_vis < G ** 3 and int(culled.n_occupied) == n_vis
    vis = occgrid.unpack_bits(culled.visible, G)
    assert (culled.ema[~vis] == 0).all() and torch.isinf(culled.ema[vis]).all()
    for _ in range(2):
        hashfield.update_occupancy(P, cfg, plain)
        hashfield.update_occupancy(P, cfg, culled)
        got, overflow = hashfield.update_occupancy(P, cfg, lean, visible_only=True, cap=n_vis)
        assert got is lean and overflow.dtype == torch.bool and not bool(overflow)
        assert torch.equal(culled.bits, plain.bits & culled.visible)
        assert int(culled.n_occupied) == OC.popcount(u32(culled.bits)) and 0 < int(culled.n_occupied) < int(plain.n_occupied)
        assert torch.equal(culled.ema[vis], plain.ema[vis]) and (culled.ema[~vis] == 0).all()
        assert torch.equal(lean.bits, culled.bits) and torch.equal(lean.n_occupied, culled.n_occupied) and torch.equal(lean.ema[vis], culled.ema[vis])
    _, overflow = hashfield.update_occupancy(P, cfg, lean, visible_only=True, cap=n_vis - 1)
    assert bool(overflow)
    with pytest.raises(RuntimeError, match="cull_invisible"):
        hashfield.update_occupancy(P, cfg, plain, visible_only=True)


@pytest.mark.parametrize("G", [8, 6])
def test_a_culled_cascade_stays_culled_and_keeps_its_parents(G):
    """K = 4: the same, with hashfield.update_occupancy_cascade; the visible set is raised so that a coarse bit stays set wherever one of its
    eight children is (G = 6: no multiple of 4, the children straddle the parents' faces)"""
    from lab4d_amd import hashfield
    P, cfg = field_fixture()
    K = 4
    base = (P["aabb"] / 8).cpu().numpy()
    aabbs = CC.cascade_boxes(K, base)
    assert np.array_equal(aabbs[K - 1], P["aabb"].cpu().numpy().reshape(6))
    thresh = median_density(P, cfg, occgrid.OccupancyCascade(dev(base), K=K, G=G))
    groups, planes_np = views(tuple(base.reshape(-1).tolist()))
    planes = dev(planes_np)
    plain, culled, lean = (occgrid.OccupancyCascade(dev(base), K=K, G=G, thresh=thresh) for _ in range(3))
    assert culled.cull_invisible(planes) is culled and lean.cull_invisible(planes) is lean
    marked = VC.unpack_levels(VC.host_mark(VC.build_host(), planes_np, aabbs, G, 1)[0], G)
    want_vis = VC.raise_to_parents(marked)
    vis_np = VC.unpack_levels(u32(culled.visible), G)
    assert np.array_equal(vis_np, want_vis) and CC.parents_hold(vis_np)
    assert culled.n_visible.cpu().tolist() == want_vis.reshape(K, -1).sum(1).tolist() == culled.n_occupied.cpu().tolist()
    assert 0 < want_vis.sum() < K * G ** 3
    grid = culled.level_grid(2)
    assert grid.visible.data_ptr() == culled.visible[2].data_ptr() and grid.n_visible.data_ptr() == culled.n_visible[2:3].data_ptr()
    vis = occgrid.unpack_bits(culled.visible, G)
    need = lean.refresh_set()
    assert need.dtype == torch.bool and bool((need | ~vis).all())
    cap = int(need.sum())
    for _ in range(2):
        hashfield.update_occupancy_cascade(P, cfg, plain)
        hashfield.update_occupancy_cascade(P, cfg, culled)
        got, overflow = hashfield.update_occupancy_cascade(P, cfg, lean, visible_only=True, cap=cap)
        assert got is lean and not bool(overflow)
        assert torch.equal(culled.bits, plain.bits & culled.visible)
        bits_np = VC.unpack_levels(u32(culled.bits), G)
        assert CC.parents_hold(bits_np) and 0 < bits_np.sum() < VC.unpack_levels(u32(plain.bits), G).sum()
        assert culled.n_occupied.cpu().tolist() == bits_np.reshape(K, -1).sum(1).tolist()
        assert torch.equal(culled.ema[vis], plain.ema[vis]) and (culled.ema[~vis] == 0).all()
        assert torch.equal(lean.bits, culled.bits) and torch.equal(lean.n_occupied, culled.n_occupied) and torch.equal(lean.ema[vis], culled.ema[vis])
    assert bool(hashfield.update_occupancy_cascade(P, cfg, lean, visible_only=True, cap=cap - 1)[1])


# ---------------------------------------------------------------------------------------------------
# the cull costs a training ray nothing
# ---------------------------------------------------------------------------------------------------
def camera_rays(groups, far_default, step=5):
    """Rays of the views themselves: pixel centres strictly inside the image, dir = Kinv (u, v, 1) in the field's frame (so t is depth),
    t_range = [near (1 + 1e-3), far (1 - 1e-3)]; views with a non-finite pose are left out"""
    O, D, T = [], [], []
    for g in groups:
        W, H = g["wh"]
        u, v = np.meshgrid(np.arange(0, W, step) + 0.5, np.arange(0, H, step) + 0.5, indexing="ij")
        for Kmat, E in zip(g["Kmat"], g["E"]):
            if not np.isfinite(E).all():
                continue
            R, t = E[:3, :3], E[:3, 3]
            d_cam = np.stack([(u.ravel() - Kmat[2]) / Kmat[0], (v.ravel() - Kmat[3]) / Kmat[1], np.ones(u.size)], 1)
            D.append(d_cam @ R)  # R^T d_cam
            O.append(np.tile(-R.T @ t, (u.size, 1)))
            far = far_default if g["far"] is None else g["far"]
            T.append(np.tile([g["near"] * (1 + 1e-3), far * (1 - 1e-3)], (u.size, 1)))
    return (dev(np.concatenate(a).astype(np.float32)) for a in (O, D, T))


RAY_KEYS = ("t", "deltas", "xyz", "dirs", "ray_idx", "ray_start", "ray_count", "total", "overflow")


def assert_same_list(a, b, keys=RAY_KEYS):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x.view(torch.int32), y.view(torch.uint8) if y.dtype == torch.bool
                                                  else y.view(torch.int32)), k


def test_the_cull_costs_the_cameras_own_rays_nothing():
    """march the culled and the unculled grid (packed.march) and cascade (packed.march_cone) along rays of the culling cameras: the same
    list word for word, although n_occupied has dropped strictly"""
    r = float(np.linalg.norm((OC.AABB[1] - OC.AABB[0]).astype(np.float64) / 2))
    groups, planes_np = views()
    # one grid over the base box, culled by the views inside it, the cut near plane and the finite far
    G = 32
    some = [groups[1], groups[4], groups[5]]
    o, d, tr = camera_rays(some, far_default=8.0 * r)
    occ = OC.random_occupancy(G, 2, 0.35)
    plain, culled = (occgrid.OccupancyGrid(dev(OC.AABB), G=G) for _ in range(2))
    for g in (plain, culled):
        g.bits.copy_(dev(OC.pack(occ).view(np.int32)))
        g.n_occupied.fill_(int(occ.sum()))
    culled.cull_invisible(dev(VC.all_planes(some)[1]))
    assert 0 < int(culled.n_occupied) < int(plain.n_occupied)
    dt, cap = 0.004, 1 << 18
    a, b = packed.march(plain, o, d, tr, dt, cap, k_max=512), packed.march(culled, o, d, tr, dt, cap, k_max=512)
    assert 1000 < int(a.total) <= cap
    assert_same_list(a, b)
    # the cascade, culled by every view
    K = 4
    o, d, tr = camera_rays(groups, far_default=30.0 * r)
    occ = CC.cascade_occupancy(K, G, 4, "random")
    plain, culled = (occgrid.OccupancyCascade(dev(OC.AABB), K=K, G=G) for _ in range(2))
    for c in (plain, culled):
        c.bits.copy_(dev(CC.pack_levels(occ).view(np.int32)))
        c.n_occupied.copy_(dev(occ.reshape(K, -1).sum(1).astype(np.int32)))
    culled.cull_invisible(dev(planes_np))
    assert (culled.n_occupied <= plain.n_occupied).all() and int(culled.n_occupied.sum()) < int(plain.n_occupied.sum())
    a = packed.march_cone(plain, o, d, tr, 1.0 / 256.0, 0.004, 0.064, cap, k_max=512)
    b = packed.march_cone(culled, o, d, tr, 1.0 / 256.0, 0.004, 0.064, cap, k_max=512)
    assert 1000 < int(a.total) <= cap
    assert_same_list(a, b, RAY_KEYS + ("steps", "level"))


def test_cull_invisible_is_capturable_and_reads_the_planes_at_replay():
    lib = VC.build_host()
    K, G = 4, 8
    _, planes_np = views()
    sets = [planes_np, planes_np[::-1].copy(), np.roll(planes_np, 3, 0)[:], planes_np]
    sets[2][:6] = planes_np[9]  # (more views that see nothing)
    planes = dev(planes_np)
    casc, grid = occgrid.OccupancyCascade(dev(OC.AABB), K=K, G=G), occgrid.OccupancyGrid(dev(OC.AABB), G=G)
    aabbs = CC.cascade_boxes(K)

    def run():
        casc.cull_invisible(planes, min_views=2)
        grid.cull_invisible(planes, min_views=2)

    run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream, no parallel branches
        run()
    for p in sets:
        planes.copy_(dev(p))
        for t in (casc.visible, casc.n_visible, grid.visible, grid.n_visible):
            t.zero_()
        casc.bits.fill_(-1)
        grid.bits.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        marked, n_marked = VC.host_mark(lib, p, aabbs, G, 2)
        want = VC.raise_to_parents(VC.unpack_levels(marked, G))
        assert np.array_equal(u32(casc.visible), CC.pack_levels(want)) and np.array_equal(u32(casc.bits), CC.pack_levels(want))
        assert casc.n_visible.cpu().tolist() == casc.n_occupied.cpu().tolist() == want.reshape(K, -1).sum(1).tolist()
        assert np.array_equal(u32(grid.visible), marked[0]) and np.array_equal(u32(grid.bits), marked[0])
        assert grid.n_visible.cpu().tolist() == grid.n_occupied.cpu().tolist() == n_marked[:1].tolist()
