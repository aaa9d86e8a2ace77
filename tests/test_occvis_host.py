"""CPU twin of the visibility cull (tests/host_harness/occvis/occvis_host.cpp over lab4d_amd/csrc/occvis_math.hpp) against the rule of
include/lab4d_occvis.h restated in numpy float64 (tests/occvis_checks.py): the SEES decision per (cell, view) inside the band the slack
allows, the guarantee that every point a view sees lies in a kept cell, camera_planes to the last bit, APPLY, and the argument checks that
need no GPU.  The GPU suite holds the kernels to this twin (tests/test_gpu_zzzzzzzzzzzzzzzzzoccvis.py).  No GPU."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conemarch_checks as CC  # noqa: E402
import occgrid_checks as OC  # noqa: E402
import occvis_checks as VC  # noqa: E402


@functools.lru_cache(None)
def views():
    groups = VC.camera_groups()
    p64, p32 = VC.all_planes(groups)
    return groups, p64, p32


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("G", [2, 5, 32, 48])
def test_twin_decides_as_the_float64_rule_outside_the_slack(K, G):
    """per (cell, view): seen where every float64 plane value is >= 0, not seen where one is < -2 slack, either in between -- and the share
    in between is <= 1 % of the pairs; the marks for min_views = 1, 2, 3 are the counts of the twin's own decisions, which lie between
    the sure count and the sure-plus-undecided count"""
    lib = VC.build_host()
    _, p64, p32 = views()
    aabbs = CC.cascade_boxes(K)
    M = p32.shape[0]
    sees = VC.host_sees(lib, p32, aabbs, G)
    sure, sure_not = VC.classify_f64(p64, aabbs, G)
    assert not (sure & sure_not).any()
    assert sees[sure].all(), int((~sees[sure]).sum())
    assert not sees[sure_not].any(), int(sees[sure_not].sum())
    undecided = ~sure & ~sure_not
    share = undecided.mean()
    print("K %d G %d: %d pairs, seen %.3f, undecided %.2e" % (K, G, sees.size, sees.mean(), share))
    assert share <= 0.01
    assert 0 < sees.mean() < 1
    nan_view = [m for m in range(M) if not np.isfinite(p32[m]).all()]
    assert len(nan_view) == 1 and not sees[:, :, nan_view[0]].any()
    away = sum(g["E"].shape[0] for g in views()[0][:2])  # the view behind the ring and the inside views looks away from every box
    assert not sees[:, :, away].any() and sees[:, :, :away].any(1).all()
    lo_count, hi_count = sure.sum(2), (sure | undecided).sum(2)
    for mv in (1, 2, 3):
        bits, n_vis = VC.host_mark(lib, p32, aabbs, G, mv)
        vis = VC.unpack_levels(bits, G).reshape(K, -1)
        assert np.array_equal(vis, sees.sum(2) >= mv)
        assert vis[lo_count >= mv].all() and not vis[hi_count < mv].any()
        assert n_vis.tolist() == [OC.popcount(w) for w in bits] == vis.sum(1).tolist()  # (the popcount of the words: the padding bits are zero)


def test_every_point_a_view_sees_lies_in_a_visible_cell():
    """20,000 random points of each level's box; a point is seen by a view if it projects into the view's image at near <= z <= far in
    float64; with min_views = 1 its cell's bit is set"""
    lib = VC.build_host()
    groups, _, p32 = views()
    K, G = 4, 32
    aabbs = CC.cascade_boxes(K)
    bits, _ = VC.host_mark(lib, p32, aabbs, G, 1)
    vis = VC.unpack_levels(bits, G)
    rng = np.random.default_rng(11)
    n_seen = 0
    for lv in range(K):
        box = aabbs[lv].reshape(2, 3)
        lo, hi = box[0].astype(np.float64), box[1].astype(np.float64)
        x01 = rng.random((20000, 3))
        pts = lo + x01 * (hi - lo)
        seen = np.concatenate([VC.points_seen_f64(pts, g) for g in groups], 1).any(1)
        cell = np.minimum((x01 * G).astype(np.int64), G - 1)
        in_vis = vis[lv][cell[:, 0], cell[:, 1], cell[:, 2]]
        assert in_vis[seen].all(), (lv, int((~in_vis[seen]).sum()))
        assert seen.any() and (lv == 0 or not vis[lv].all())
        n_seen += int(seen.sum())
    assert n_seen > 1000


def test_camera_planes_equal_the_float64_statement_to_the_last_bit():
    import torch
    from lab4d_amd import occgrid
    groups, _, _ = views()
    for g in groups:
        for E in (g["E"], g["E"][:, :3]):
            got = occgrid.camera_planes(torch.from_numpy(g["Kmat"]), torch.from_numpy(np.ascontiguousarray(E)), g["wh"], g["near"], g["far"], g["pad"])
            want = VC.planes_f64(g["Kmat"], g["E"], g["wh"], g["near"], g["far"], g["pad"]).astype(np.float32)
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape and got.is_contiguous()
            assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
        if g["far"] is None:
            assert np.array_equal(got.numpy()[:, 5], np.tile(np.float32([0, 0, 0, 1]), (got.shape[0], 1)))
        else:
            assert (got.numpy()[:, 5, 3] > 0).all() and np.allclose(np.linalg.norm(got.numpy()[:, 5, :3], axis=1), 1)
    # fp32 inputs are taken to float64 first; unit normals; a point in front of a ring camera, on its axis, is inside all six half-spaces
    g = groups[0]
    got = occgrid.camera_planes(torch.from_numpy(g["Kmat"]).float(), torch.from_numpy(g["E"]).float(), g["wh"], g["near"]).numpy().astype(np.float64)
    assert np.allclose(np.linalg.norm(got[:, :5, :3], axis=2), 1, atol=1e-6)
    mid = (OC.AABB[0].astype(np.float64) + OC.AABB[1]) / 2
    assert (got[:, :, :3] @ mid + got[:, :, 3] > 0).all()
    # pad widens the frustum: every side plane moves outwards (its value grows at any point in front of the camera), near and far stay
    a = VC.planes_f64(g["Kmat"], g["E"], g["wh"], g["near"], 3.0, 0.0)
    b = occgrid.camera_planes(torch.from_numpy(g["Kmat"]), torch.from_numpy(g["E"]), g["wh"], g["near"], 3.0, 8.0).numpy().astype(np.float64)
    assert ((b[:, :4, :3] @ mid + b[:, :4, 3]) > (a[:, :4, :3] @ mid + a[:, :4, 3])).all()
    assert np.allclose(a[:, 4:], b[:, 4:], atol=1e-6)
    with pytest.raises(RuntimeError, match="camera_planes"):
        occgrid.camera_planes(torch.zeros(2, 3), torch.zeros(2, 4, 4), (4, 4), 0.1)
    with pytest.raises(RuntimeError, match="camera_planes"):
        occgrid.camera_planes(torch.zeros(2, 4), torch.zeros(3, 4, 4), (4, 4), 0.1)


@pytest.mark.parametrize("K,G", [(1, 5), (4, 8)])
def test_apply_twin_clears_the_invisible_cells(K, G):
    lib = VC.build_host()
    rng = np.random.default_rng(3)
    occ, vis = rng.random((K, G, G, G)) < 0.5, rng.random((K, G, G, G)) < 0.6
    bits, vbits = CC.pack_levels(occ), CC.pack_levels(vis)
    ema0 = np.stack([OC.density_volume(G, 5 + c) for c in range(K)])
    ema = ema0.copy()
    n = VC.host_apply(lib, vbits, ema, bits, G)
    assert np.array_equal(bits, CC.pack_levels(occ & vis)) and n.tolist() == (occ & vis).reshape(K, -1).sum(1).tolist()
    v = vis.reshape(K, -1)
    assert (ema[~v] == 0).all() and np.array_equal(ema[v].view(np.uint32), ema0[v].view(np.uint32))


def test_argument_rules_are_rejected_before_a_launch():
    """the library's own checks run before any launch, so they need no GPU; lab4d_amd.occgrid imports without one, and its Python checks
    refuse what they can before they touch the device"""
    import torch
    from lab4d_amd import _lib, hashfield, occgrid
    _lib.build(verbose=False)
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    good = dict(M=8, K=4, G=32, mv=1)
    bad = [(dict(M=0), b"M = 0 "), (dict(M=-3), b"M = -3 "), (dict(M=(1 << 20) + 1), b"M = 1048577 "), (dict(K=0), b"K = 0 "), (dict(K=9), b"K = 9 "),
           (dict(G=1), b"G = 1 "), (dict(G=257), b"G = 257 "), (dict(mv=0), b"min_views = 0 "), (dict(mv=9), b"min_views = 9 "), (dict(mv=-1), b"min_views = -1 ")]
    for change, word in bad:
        a = dict(good, **change)
        assert lib.lab4d_occvis_mark(p, a["M"], p, a["K"], a["G"], a["mv"], p, p, None) == -1, change
        assert word in lib.lab4d_last_error(), (change, lib.lab4d_last_error())
    for K, G, word in ((0, 32, b"K = 0 "), (9, 32, b"K = 9 "), (1, 1, b"G = 1 "), (1, 300, b"G = 300 ")):
        assert lib.lab4d_occvis_apply(p, p, p, p, K, G, None) == -1
        assert word in lib.lab4d_last_error()
    for args in ((None, 8, p, 4, 32, 1, p, p), (p, 8, None, 4, 32, 1, p, p), (p, 8, p, 4, 32, 1, None, p), (p, 8, p, 4, 32, 1, p, None)):
        assert lib.lab4d_occvis_mark(*args, None) == -1 and b"null" in lib.lab4d_last_error()
    assert lib.lab4d_occvis_mark(ctypes.c_void_p(p.value + 4), 8, p, 4, 32, 1, p, p, None) == -1 and b"aligned" in lib.lab4d_last_error()
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.lab4d_occvis_apply(*args, 4, 32, None) == -1 and b"null" in lib.lab4d_last_error()
    # the Python layer
    grid = occgrid.OccupancyGrid.__new__(occgrid.OccupancyGrid)
    grid.G, grid.aabb = 8, torch.zeros(2, 3)
    assert grid.visible is None and grid.n_visible is None
    with pytest.raises(RuntimeError, match="no CPU path"):
        grid.cull_invisible(torch.zeros(2, 6, 4))
    P, cfg = hashfield.make_weights(0, {"L": 16, "F": 2, "log2_T": 10, "n_min": 4, "n_max": 32})
    grid.cell_centers = lambda: torch.zeros(512, 3)
    with pytest.raises(RuntimeError, match="cull_invisible"):
        hashfield.update_occupancy(P, cfg, grid, visible_only=True)
    grid.visible = torch.zeros(16, dtype=torch.int32)
    for cap in (None, 0):
        with pytest.raises(RuntimeError, match="needs cap"):  # a static capacity is required: all G^3 rows would save nothing
            hashfield.update_occupancy(P, cfg, grid, visible_only=True, cap=cap)
