"""The occupancy grid of the hash field on the CPU: the twin of the kernels (tests/host_harness/occgrid_host.cpp, the same
csrc/occgrid_math.hpp functions) against the rules of include/lab4d_occgrid.h restated in numpy float64 (tests/occgrid_checks.py).  The
reference has no occupancy grid, so these rules are the definition; the GPU suite (tests/test_gpu_zzzzoccgrid.py) then holds the kernels
bit for bit to this twin.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occgrid_checks as OC  # noqa: E402

import lab4d_amd.occgrid  # noqa: E402,F401  (the feature under test: its host layer must import without a GPU)


@pytest.fixture(scope="module")
def host():
    return OC.build_host()


@pytest.mark.parametrize("G", [2, 5, 32, 48])
def test_bit_layout(host, G):
    """cell idx = (i*G + j)*G + k is bit idx & 31 of word idx >> 5, for every cell on its own; the padding bits stay zero"""
    n = G ** 3
    rng = np.random.default_rng(G)
    cells = np.arange(n) if n <= 125 else np.unique(np.concatenate([rng.integers(0, n, 200), [0, 31, 32, n - 1]]))
    ema, bits, _ = OC.host_init(host, G)
    for idx in cells:
        dens = np.zeros(n, np.float32)
        dens[idx] = 1.0
        assert OC.host_update(host, dens, ema, bits, G, 0.0, 0.5) == 1  # decay 0: the ema is the fresh density
        assert bits.size == (n + 31) // 32
        assert bits[idx >> 5] == np.uint32(1) << np.uint32(idx & 31), idx
        assert OC.popcount(bits) == 1, idx
    # every cell at once: all bits of the grid, none of the padding
    assert OC.host_update(host, np.ones(n, np.float32), ema, bits, G, 0.0, 0.5) == n
    assert np.array_equal(bits, OC.pack(np.ones((G, G, G), bool)))
    if n % 32:
        assert bits[-1] == (1 << (n % 32)) - 1
    # the mask kernel's lookup uses the same layout: a point at the centre of cell (i, j, k)
    occ = OC.random_occupancy(G, 11, 0.3)
    ijk = np.stack(np.meshgrid(*[np.arange(G)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = OC.to_world((ijk + 0.5) / G)
    assert np.array_equal(OC.host_mask(host, centres, OC.AABB, OC.pack(occ), G).astype(bool), occ.reshape(-1))


@pytest.mark.parametrize("G", [5, 32])
def test_update_rule(host, G):
    n = G ** 3
    ema, bits, n_occ = OC.host_init(host, G)
    assert np.isposinf(ema).all() and n_occ == n and np.array_equal(bits, OC.pack(np.ones((G, G, G), bool)))  # a fresh grid is all ones
    decay, thresh = np.float32(0.95), np.float32(0.01)
    expect = np.full(n, np.inf, np.float32)
    for it in range(3):
        dens = OC.density_volume(G, 100 * G + it)
        with np.errstate(invalid="ignore"):
            d = np.where(dens > 0, dens, np.float32(0)).astype(np.float32)  # NaN and negative count as 0
        expect = np.where(np.isposinf(expect), d, np.maximum((expect * decay).astype(np.float32), d))  # an update of +inf replaces it
        n_occ = OC.host_update(host, dens, ema, bits, G, float(decay), float(thresh))
        assert np.array_equal(ema.view(np.uint32), expect.view(np.uint32)), it
        assert np.array_equal(OC.unpack(bits, G).reshape(-1), expect > thresh), it
        assert n_occ == OC.popcount(bits) == int((expect > thresh).sum()), it
    assert 0 < n_occ < n and np.isposinf(expect).sum() >= 1  # (+inf density: the cell is back to "nothing known")
    # a cell that saw density once decays below the threshold in the expected number of steps, never earlier
    ema2, bits2, _ = OC.host_init(host, 2)
    OC.host_update(host, np.full(8, 0.02, np.float32), ema2, bits2, 2, float(decay), float(thresh))
    e, steps = np.float32(0.02), 0
    while e > thresh:
        assert OC.popcount(bits2) == 8
        OC.host_update(host, np.zeros(8, np.float32), ema2, bits2, 2, float(decay), float(thresh))
        e, steps = np.float32(e * decay), steps + 1
    assert OC.popcount(bits2) == 0 and steps == 14  # 0.02 * 0.95^14 = 0.00975


@pytest.mark.parametrize("G", [5, 48])
def test_mask_rule(host, G):
    sp, sp_in = OC.special_points()
    ones = OC.pack(np.ones((G, G, G), bool))
    assert np.array_equal(OC.host_mask(host, sp, OC.AABB, ones, G).astype(bool), sp_in)  # faces in, the next float out, NaN out
    # the corners sit in the corner cells: with only those 8 bits set they still pass, with only those 8 cleared they do not
    corners = np.zeros((G, G, G), bool)
    corners[::G - 1, ::G - 1, ::G - 1] = True
    assert OC.host_mask(host, sp[:8], OC.AABB, OC.pack(corners), G).all()
    assert not OC.host_mask(host, sp[:8], OC.AABB, OC.pack(~corners), G).any()
    # random points against the float64 rule, wherever float32 x01 * G is farther than 1e-4 from an integer
    occ = OC.random_occupancy(G, 3, 0.4)
    pts = OC.mask_points(64 * 1000 + 1, 17)[sp.shape[0]:]
    ref, clear64 = OC.ref_mask(pts, occ, G)
    x01_32 = (pts - OC.AABB[0]) / (OC.AABB[1] - OC.AABB[0])
    q32 = x01_32 * np.float32(G)
    clear = (np.abs(q32 - np.round(q32)) > OC.MARGIN).all(-1)
    left_out = 1 - clear.mean()
    assert 1 - clear64.mean() <= 0.01  # the reference rule's own share stays under the cap: the points were drawn for it
    print("mask G=%d: %.4f %% of the points left out by the face margin" % (G, 100 * left_out))
    assert left_out <= 0.01
    got = OC.host_mask(host, pts, OC.AABB, OC.pack(occ), G).astype(bool)
    assert np.array_equal(got[clear], ref[clear]), int((got[clear] != ref[clear]).sum())
    assert 0.1 < ref.mean() < 0.4  # (both answers occur: 58 % of the points lie in the box, 40 % of the cells are set)


@pytest.fixture(scope="module")
def ray_set():
    return OC.rays(5)


@pytest.mark.parametrize("G,kind", [(8, "random"), (8, "sphere"), (48, "random"), (48, "sphere")])
def test_ray_span_is_conservative_and_tight(host, ray_set, G, kind):
    o, d, tr, kinds = ray_set
    occ = OC.random_occupancy(G, 7) if kind == "random" else OC.sphere_occupancy(G)
    span, hit, steps = OC.host_ray_span(host, o, d, tr, OC.AABB, OC.pack(occ), G)
    hit = hit.astype(bool)
    assert steps.max() <= 3 * G and steps.min() >= 0
    assert np.isfinite(span).all()
    t0, t1 = tr[:, 0], tr[:, 1]
    assert (span[:, 0] >= t0).all() and (span[:, 1] <= t1).all() and (span[:, 0] <= span[:, 1]).all()
    assert np.array_equal(span[~hit], np.stack([t0, t0], 1)[~hit])  # no hit: both outputs equal t0
    # conservative: every float64 sample inside an occupied cell (clear of the faces) lies in the span
    t, good, n_margin = OC.ref_ray_samples(o, d, tr, occ, G)
    share = n_margin / good.size
    print("ray_span G=%d %s: %.4f %% of the (ray, t) pairs left out by the face margin; %d of %d rays hit" % (G, kind, 100 * share, hit.sum(), hit.size))
    assert share <= 0.01
    inside = (t >= span[:, :1].astype(np.float64)) & (t <= span[:, 1:].astype(np.float64)) & hit[:, None]
    assert not (good & ~inside).any(), np.nonzero((good & ~inside).any(1))[0][:10]
    # hit = 0 iff no such t exists: a ray with one has hit = 1 (above); a ray without a hit has none, and a ray whose float64 walk meets no
    # occupied cell at all has no hit
    assert not good[~hit].any()
    entry, exit_, occd = OC.ref_walk(o, d, tr, occ, G)
    assert not hit[~occd.any(1)].any()
    # tight: t_first / t_last within one cell diagonal of the float64 entry / exit of an occupied cell on the ray
    diag = OC.cell_diagonal_t(d, G)
    far = np.where(occd, 0.0, np.inf)
    e_first = np.min(np.abs(entry - span[:, :1]) + far, 1)
    e_last = np.min(np.abs(exit_ - span[:, 1:]) + far, 1)
    assert (e_first[hit] <= diag[hit]).all() and (e_last[hit] <= diag[hit]).all(), (float((e_first[hit] / diag[hit]).max()), float((e_last[hit] / diag[hit]).max()))
    # every kind of ray does what it was built for
    assert not hit[kinds["miss"]].any()
    if kind == "sphere":
        assert hit[kinds["diagonal"]].all() and hit[kinds["random"]].mean() > 0.2
        for name in ("axis", "inside", "t1_inside", "negative"):
            assert 0 < hit[kinds[name]].sum() < hit[kinds[name]].size, name


def test_ray_span_refuses_malformed_rays(host):
    """non-finite inputs, t0 > t1 and an empty box: no hit, t_span = (t0, t0), and the walk does not even start"""
    G = 8
    ones = OC.pack(np.ones((G, G, G), bool))
    o = np.tile(OC.to_world([[-0.5, 0.5, 0.5]]), (6, 1))
    d = np.tile(np.array([[0.3, 0.0, 0.0]], np.float32), (6, 1))
    tr = np.tile(np.array([[0.0, 10.0]], np.float32), (6, 1))
    o[1, 1] = np.nan
    d[2, 0] = np.inf
    tr[3] = [2.0, 1.0]
    tr[4, 1] = np.inf
    d[5, 0] = 1e-44  # 1 / d01 overflows: treated as parallel; the origin is outside that slab
    span, hit, steps = OC.host_ray_span(host, o, d, tr, OC.AABB, ones, G)
    assert hit.tolist() == [1, 0, 0, 0, 0, 0] and steps[1:].max() == 0 and steps[0] == G
    assert np.array_equal(span[1:], np.stack([tr[1:, 0], tr[1:, 0]], 1))
    empty = np.array([[0, 0, 0], [1, 0, 1]], np.float32)
    span, hit, steps = OC.host_ray_span(host, o[:1], d[:1], tr[:1], empty, ones, G)
    assert not hit.any() and steps.max() == 0
    assert not OC.host_mask(host, np.zeros((1, 3), np.float32), empty, ones, G).any()


def test_host_layer_refuses_cpu_tensors():
    import torch
    from lab4d_amd import occgrid
    with pytest.raises(RuntimeError, match="no CPU path"):
        occgrid.OccupancyGrid(torch.tensor(OC.AABB), G=8)
