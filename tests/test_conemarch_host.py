"""CPU twin of the cone-stepped march through a cascade of occupancy grids (tests/host_harness/conemarch/conemarch_host.cpp over
lab4d_amd/csrc/conemarch_math.hpp) against the rules of include/lab4d_conemarch.h restated in numpy (tests/conemarch_checks.py): word for
word in float32, the kept set in float64, the properties of the recurrence, the cascade's propagation rule, the sanitizers, and the argument
checks that need no GPU.  The GPU suite holds the kernels to this twin (tests/test_gpu_zzzzzzzzzzzzzzzzconemarch.py); here the twin itself is
pinned.  No GPU."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conemarch_checks as CC  # noqa: E402
import host_twin  # noqa: E402
import occgrid_checks as OC  # noqa: E402

# every K, G, R, k_max and cone of the list at least once, each K with each G
CASES = [(1, 4, 1025, 64, 0.05), (1, 32, 65, 200, 0.0), (2, 4, 65, 65, 1.0 / 256.0), (2, 32, 1025, 1, 0.05), (4, 4, 1025, 200, 1.0 / 256.0),
         (4, 32, 1025, 64, 0.0), (4, 32, 1, 65, 0.05), (4, 4, 65, 200, 0.05)]


def _caps(res):
    cnt, total = res["count"], res["total"]
    inside = next((int(res["ray_start"][r]) + 1 for r in range(len(cnt)) if cnt[r] >= 2), 0)  # a cut inside a ray
    return sorted({total, max(total - 1, 0), inside, 0})


@pytest.mark.parametrize("K,G,R,k_max,cone", CASES)
def test_twin_equals_the_numpy_float32_rules_word_for_word(K, G, R, k_max, cone):
    """t, steps, deltas, xyz and dirs by their words, level, the counts, total, overflow, the parked rows and the sentinels behind the cap, on
    the special rays (tests/conemarch_checks.py ray_set), with a random and a ball cascade, at the capacities total, total - 1, a cut inside a
    ray and 0"""
    lib = CC.build_host()
    aabbs = CC.cascade_boxes(K)
    o, d, tr, kinds = CC.ray_set(aabbs)
    o, d, tr = o[:R], d[:R], tr[:R]
    n_rows = 0
    for kind in ("random", "ball"):
        occ = CC.cascade_occupancy(K, G, 3, kind)
        bits = CC.pack_levels(occ)
        full = CC.host_march(lib, o, d, tr, aabbs, bits, G, cone, CC.DT_MIN, CC.DT_MAX, k_max)
        for cap in _caps(full):
            got = CC.host_march(lib, o, d, tr, aabbs, bits, G, cone, CC.DT_MIN, CC.DT_MAX, k_max, cap=cap, tail=3)
            ref = CC.f32_march(o, d, tr, aabbs, occ, G, cone, CC.DT_MIN, CC.DT_MAX, k_max, cap=cap, tail=3)
            CC.assert_same(got, ref, (K, G, R, k_max, cone, kind, cap))
            n = min(cap, got["total"])
            assert (got["ray_idx"][n:cap] == -1).all() and (got["level"][n:cap] == -1).all() and (got["ray_idx"][cap:] == -7).all()
            assert np.isnan(got["t"][cap:]).all() and got["ray_count"].sum() == n
        n_rows += full["total"]
        cnt = full["count"]
        assert (cnt[2:min(R, 10)] == 0).all()  # non-finite inputs, t0 > t1
        if R > 13:
            assert cnt[12] == 0 and cnt[13] == 0  # a miss of box K - 1, |d| = 0
        if R == 1025:
            assert (cnt[kinds["miss"]] == 0).all()
    assert n_rows > (0 if k_max == 1 and R == 1 else 1)
    print("K = %d, G = %d, R = %d, k_max = %d, cone = %g: %d rows" % (K, G, R, k_max, cone, n_rows))


@pytest.mark.parametrize("K,G", [(1, 32), (2, 4), (4, 4), (4, 32)])
def test_cascade_mask_twin_equals_the_numpy_float32_rule(K, G):
    lib = CC.build_host()
    aabbs = CC.cascade_boxes(K)
    occ = CC.cascade_occupancy(K, G, 11)
    pts, delta = CC.mask_points(4097, 7, aabbs)
    edges = CC.f32_edges(aabbs, G)
    delta[:K], delta[K], delta[K + 1], delta[K + 2] = edges, 0.0, np.nan, np.inf  # exactly an edge (kept at that level: <=), and the odd ones
    for dl in (delta, None):
        mask, level = CC.host_cascade_mask(lib, pts, dl, aabbs, CC.pack_levels(occ), G)
        kept, lv = CC.f32_level_rule(pts, np.zeros(len(pts), np.float32) if dl is None else dl, aabbs, occ, G)
        assert np.array_equal(mask, kept.astype(np.uint8)) and np.array_equal(level, lv.astype(np.int32))
        assert (level >= -1).all() and (level < K).all() and (mask[level < 0] == 0).all()
        assert 0 < mask.sum() < len(pts) and (level == -1).sum() > 0
    if K > 1:
        assert len(np.unique(level)) == K + 1  # (without delta: every level is some point's c_pos)


@pytest.mark.parametrize("K,G,cone", [(1, 32, 0.05), (2, 32, 0.0), (4, 32, 1.0 / 256.0), (4, 4, 0.05), (4, 32, 0.05)])
def test_kept_set_equals_the_float64_classification(K, G, cone):
    """The twin's kept rows against the LEVEL rule with the points, steps, edges and cells in float64, on every candidate where x01 * G is
    farther than 1e-4 from an integer on all axes at the level used and delta is farther than a relative 1e-5 from every edge.  The excluded
    share is asserted below 1 %; measured on the CPU: 2.8e-4 to 8.7e-4 at G = 32 (K = 1 / 2 / 4), 6.3e-4 at G = 4."""
    lib = CC.build_host()
    aabbs = CC.cascade_boxes(K)
    o, d, tr = CC.generic_rays(600, 31 + K + G, aabbs)
    k_max = 200
    n_kept = 0
    for kind in ("random", "ball"):
        occ = CC.cascade_occupancy(K, G, 5, kind)
        res = CC.host_march(lib, o, d, tr, aabbs, CC.pack_levels(occ), G, cone, CC.DT_MIN, CC.DT_MAX, k_max)
        c = CC.f32_candidates(o, d, tr, aabbs, cone, CC.DT_MIN, CC.DT_MAX, k_max)
        keep, level, clear = CC.f64_classification(o, d, c, aabbs, occ, G)
        kept = np.zeros(c["t"].shape, bool)
        # every emitted t must BE a candidate of its ray: place the rows by their words
        r = res["ray_idx"].astype(np.int64)
        for ray in np.unique(r):
            rows = np.nonzero(r == ray)[0]
            k = np.searchsorted(c["t"][ray][c["cand"][ray]], res["t"][rows])
            assert np.array_equal(c["t"][ray][k], res["t"][rows]) and len(np.unique(k)) == len(k)
            kept[ray, k] = True
        assert kept.sum() == res["total"] and not (kept & ~c["cand"]).any()
        look = c["cand"] & clear
        assert np.array_equal(kept[look], keep[look]), int((kept[look] != keep[look]).sum())
        rr, kk = np.nonzero(kept & look)
        assert np.array_equal(level[rr, kk], res["level"][np.nonzero((kept & look)[kept])[0]])  # and at the same level
        excluded = float((c["cand"] & ~clear).sum()) / float(c["cand"].sum())
        print("K = %d, G = %d, cone = %g, %s: %d candidates, %d kept, share excluded %.2e" % (K, G, cone, kind, c["cand"].sum(), kept.sum(), excluded))
        assert excluded < 0.01, excluded
        n_kept += int(kept.sum())
    assert n_kept > 2000


@pytest.mark.parametrize("K,G,cone", [(1, 4, 0.0), (1, 32, 0.05), (4, 32, 0.0), (4, 4, 1.0 / 256.0), (4, 32, 0.05)])
def test_properties_of_the_march(K, G, cone):
    lib = CC.build_host()
    aabbs = CC.cascade_boxes(K)
    o, d, tr, _ = CC.ray_set(aabbs)
    k_max = 200
    fresh = CC.host_march(lib, o, d, tr, aabbs, CC.pack_levels(CC.cascade_occupancy(K, G, 0, "full")), G, cone, CC.DT_MIN, CC.DT_MAX, k_max)
    c = CC.f32_candidates(o, d, tr, aabbs, cone, CC.DT_MIN, CC.DT_MAX, k_max)
    f = np.float32
    # the intervals tile the ray from t_in: a_0 = t_in, a_{k+1} = a_k + s_k, t_k = a_k + s_k / 2 -- on the rows of a fresh cascade, which keeps
    # every candidate that has a cell in box K - 1: the rows of a ray ARE its candidates, in order
    has, _ = CC.f32_cells(c["p"].reshape(-1, 3), aabbs[K - 1], G)
    in_outer = has.reshape(c["t"].shape) & c["cand"]
    assert np.array_equal(fresh["count"], in_outer.sum(1)) and fresh["total"] > 1000
    starts = fresh["ray_start"]
    for ray in np.nonzero(fresh["count"])[0][:200]:
        rows = slice(starts[ray], starts[ray] + fresh["count"][ray])
        k = np.nonzero(in_outer[ray])[0]
        t, s = fresh["t"][rows], fresh["steps"][rows]
        assert np.array_equal(t, c["t"][ray, k]) and np.array_equal(s, c["s"][ray, k])
        a = c["a"][ray]
        assert a[0] == c["t_in"][ray]
        n = int(c["cand"][ray].sum())
        assert np.array_equal(a[1:n], (a[:n - 1] + c["s"][ray, :n - 1]).astype(f))
        assert np.array_equal(c["t"][ray, :n], (a[:n] + (f(0.5) * c["s"][ray, :n]).astype(f)).astype(f))
        assert (np.diff(t) > 0).all()  # ascending within a ray
        if c["t_in"][ray] >= 0:
            assert (np.diff(c["s"][ray, :n]) >= 0).all()  # the step does not decrease with k
        else:
            assert c["s"][ray, 0] == f(CC.DT_MIN)  # t0 < 0: the step clamps to dt_min
    assert -1 <= c["t_in"][10] < 0 and fresh["count"][10] > 0 and fresh["steps"][starts[10]] == f(CC.DT_MIN)  # (t0 = -1, or where the box begins)
    n = fresh["total"]
    assert ((fresh["steps"][:n] >= f(CC.DT_MIN)) & (fresh["steps"][:n] <= f(CC.DT_MAX))).all()
    if cone == 0.0:
        assert (fresh["steps"][:n] == f(CC.DT_MIN)).all()
    else:
        assert len(np.unique(fresh["steps"][:n])) > 2
    r = fresh["ray_idx"].astype(np.int64)
    assert np.array_equal(fresh["deltas"], (fresh["steps"] * c["len"][r]).astype(f))
    assert np.array_equal(fresh["ray_idx"], np.repeat(np.arange(len(o), dtype=np.int32), fresh["count"]))
    # level >= c_pos on every row; K = 1 never reports another level than 0
    _, c_pos = CC.f32_level_rule(fresh["xyz"], np.zeros(n, f), aabbs, CC.cascade_occupancy(K, G, 0, "full"), G)
    assert (c_pos >= 0).all() and (fresh["level"] >= c_pos).all() and (fresh["level"] < K).all()
    if K == 1:
        assert (fresh["level"] == 0).all()
    else:
        assert len(np.unique(fresh["level"])) >= 2
    # an all-empty cascade keeps nothing
    none = CC.host_march(lib, o, d, tr, aabbs, CC.pack_levels(CC.cascade_occupancy(K, G, 0, "empty")), G, cone, CC.DT_MIN, CC.DT_MAX, k_max, cap=5)
    assert none["total"] == 0 and not none["overflow"] and (none["ray_count"] == 0).all() and (none["ray_idx"] == -1).all()
    no_rays = CC.host_march(lib, o[:0], d[:0], tr[:0], aabbs, CC.pack_levels(CC.cascade_occupancy(K, G, 0, "full")), G, cone, CC.DT_MIN, CC.DT_MAX, k_max, cap=4)
    assert no_rays["total"] == 0 and not no_rays["overflow"] and (no_rays["ray_idx"] == -1).all()


@pytest.mark.parametrize("G", [4, 32, 6])
def test_propagation_keeps_every_parent_bit_set(G):
    """The numpy update rule only: after any sequence of updates with random densities, NaN and negative values included, every set bit of
    level c - 1 has its parent bit set at level c (K = 3; G = 6: the cells of a level straddle the faces of the next)"""
    K, decay, thresh = 3, 0.5, 0.01  # (a fast decay: bits go off again within the eight updates)
    ema = CC.np_cascade_new(K, G)
    rng = np.random.default_rng(G)
    seen = set()
    for step in range(8):
        dens = CC.cascade_density(K, G, 100 * step + G)
        if step % 3 == 2:
            dens[rng.integers(K)] = 0.0  # a level that sees nothing this time: only the decay and what comes up from below
        occ = CC.np_cascade_update(ema, dens, K, G, decay, thresh)
        assert CC.parents_hold(occ), step
        j = CC.parent_index(G)
        pooled = np.zeros((G, G, G), np.float32)
        np.maximum.at(pooled, tuple(np.meshgrid(j, j, j, indexing="ij")), ema[0].reshape(G, G, G))
        assert (ema[1].reshape(G, G, G) >= pooled).all()  # the invariant behind it
        seen.add((int(occ[0].sum()), int(occ[2].sum())))
        assert occ[0].sum() > 0
    assert len(seen) > 1 and min(n for n, _ in seen) < G ** 3
    # and the rule does something: without the propagation the property fails on the same densities
    ema0 = CC.np_cascade_new(K, G)
    dens = CC.cascade_density(K, G, 1)
    plain = np.stack([np.where(dens[c] > 0, dens[c], 0) > thresh for c in range(K)]).reshape(K, G, G, G)
    assert not CC.parents_hold(plain) and CC.parents_hold(CC.np_cascade_update(ema0, dens, K, G, decay, thresh))


def test_twin_runs_clean_under_the_sanitizers():
    """the stand-alone program over the truncation cases, the rays without samples and K = 1 / 4, AddressSanitizer +
    UndefinedBehaviorSanitizer, on the CPU"""
    r = subprocess.run([host_twin.sanitized_main("conemarch")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "conemarch_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_every_argument_rule_is_rejected_before_a_launch():
    """the library's own checks run before any launch, so they need no GPU: every ARGUMENTS rule of include/lab4d_conemarch.h, on both march
    calls and (K and G) on the per-point call; then the Python layer's, which refuses the same scalars before it looks at a tensor"""
    import torch
    from lab4d_amd import _lib, packed
    _lib.build(verbose=False)
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    inf, nan = float("inf"), float("nan")
    good = dict(K=4, G=32, R=4, cone=0.01, dt_min=0.01, dt_max=0.1, k_max=8, cap=16)
    bad = [(dict(cone=-0.1), b"cone"), (dict(cone=nan), b"cone"), (dict(cone=inf), b"cone"), (dict(dt_min=0.0), b"dt_min"), (dict(dt_min=nan), b"dt_min"),
           (dict(dt_min=inf, dt_max=inf), b"dt_min"), (dict(dt_max=0.005), b"dt_max"), (dict(dt_max=inf), b"dt_max"), (dict(dt_max=nan), b"dt_max"),
           (dict(k_max=0), b"k_max"), (dict(R=1 << 22, k_max=1 << 9), b"31 bits"), (dict(K=0), b"K = 0 "), (dict(K=9), b"K = 9 "), (dict(G=1), b"G = 1 "),
           (dict(G=257), b"G = 257 "), (dict(G=31), b"even"), (dict(R=-1), b"R < 0")]
    for change, word in bad:
        a = dict(good, **change)
        head = (p, p, p, p, p, a["K"], a["G"], a["R"], a["cone"], a["dt_min"], a["dt_max"], a["k_max"])
        assert lib.lab4d_packed_march_cone_count(*head, p, None) == -1, change
        assert word in lib.lab4d_last_error(), (change, lib.lab4d_last_error())
        assert lib.lab4d_packed_march_cone_write(*head, p, a["cap"], p, p, p, p, p, p, p, p, p, p, None) == -1, change
        assert word in lib.lab4d_last_error(), (change, lib.lab4d_last_error())
    for cap in (-1, 1 << 31):
        a = good
        assert lib.lab4d_packed_march_cone_write(p, p, p, p, p, a["K"], a["G"], a["R"], a["cone"], a["dt_min"], a["dt_max"], a["k_max"], p, cap, p, p, p, p, p,
                                                 p, p, p, p, p, None) == -1
        assert b"cap" in lib.lab4d_last_error()
    for K, G, word in ((0, 32, b"K = 0 "), (9, 32, b"K = 9 "), (2, 31, b"even"), (2, 1, b"G = 1 "), (1, 258, b"G = 258 ")):
        assert lib.lab4d_occgrid_cascade_mask(p, None, p, p, K, G, 4, p, None, None) == -1
        assert word in lib.lab4d_last_error()
    assert lib.lab4d_packed_march_cone_count(p, p, p, p, p, 1, 31, 0, 0.0, 0.01, 0.01, 1, p, None) == 0  # K = 1 takes an odd G; no rays: no launch
    assert lib.lab4d_occgrid_cascade_mask(p, None, p, p, 1, 31, 0, p, None, None) == 0
    # the Python layer
    o, d, tr = torch.zeros(4, 3), torch.ones(4, 3), torch.tensor([[0.0, 1.0]] * 4)
    casc = types.SimpleNamespace(K=2, G=8, aabbs=None, bits=None)
    for kw, word in [(dict(cone=-1.0), "cone"), (dict(cone=nan), "cone"), (dict(dt_min=0.0), "dt_min"), (dict(dt_min=inf), "dt_min"), (dict(dt_max=0.001), "dt_max"),
                     (dict(dt_max=inf), "dt_max"), (dict(k_max=0), "k_max"), (dict(k_max=1 << 29), "31 bits"), (dict(cap=-1), "cap"), (dict(cap=1 << 31), "cap")]:
        a = dict(dict(cone=0.01, dt_min=0.01, dt_max=0.1, cap=16, k_max=8), **kw)
        with pytest.raises(RuntimeError, match=word):
            packed.march_cone(casc, o, d, tr, a["cone"], a["dt_min"], a["dt_max"], a["cap"], k_max=a["k_max"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.march_cone(casc, o, d, tr, 0.01, 0.01, 0.1, 16)


def test_cascade_and_field_level_checks_without_a_gpu():
    import torch
    from lab4d_amd import hashfield, occgrid
    box = torch.tensor(OC.AABB)
    with pytest.raises(RuntimeError, match="even"):
        occgrid.OccupancyCascade(box, K=2, G=31)
    for K in (0, 9, -1):
        with pytest.raises(RuntimeError, match=r"K = -?\d+ outside \[1, 8\]"):
            occgrid.OccupancyCascade(box, K=K, G=32)
    for G in (1, 257):
        with pytest.raises(RuntimeError, match=r"G = \d+ outside \[2, 256\]"):
            occgrid.OccupancyCascade(box, K=1, G=G)
    with pytest.raises(RuntimeError, match="no CPU path"):  # (K = 1 takes an odd G: refused only for being on the host)
        occgrid.OccupancyCascade(box, K=1, G=31)
    # a field that does not live on the outermost box
    aabbs = torch.tensor(CC.cascade_boxes(3))
    casc = types.SimpleNamespace(K=3, G=8, aabbs=aabbs)
    P, cfg = hashfield.make_weights(0, {"L": 16, "F": 2, "log2_T": 10, "n_min": 4, "n_max": 32})
    for wrong in (aabbs[0].view(2, 3), aabbs[1].view(2, 3), aabbs[2].view(2, 3) * 1.0001, P["aabb"]):
        with pytest.raises(RuntimeError, match="outermost box"):
            hashfield.update_occupancy_cascade(dict(P, aabb=wrong), cfg, casc)
    with pytest.raises(AttributeError, match="cell_centers"):  # the right box passes the check (and then needs a real cascade)
        hashfield.update_occupancy_cascade(dict(P, aabb=aabbs[2].view(2, 3).clone()), cfg, casc)
