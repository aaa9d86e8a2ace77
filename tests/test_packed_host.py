"""CPU twin of packed marching / compositing (tests/host_harness/packed_host.cpp over lab4d_amd/csrc/packed_math.hpp) against the rules of
include/lab4d_packed.h restated in float64 (tests/packed_checks.py).  The GPU suite holds the kernels to this twin
(tests/test_gpu_zzzzzpacked.py); here the twin itself is pinned.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import occgrid_checks as OC  # noqa: E402
import packed_checks as PC  # noqa: E402

DT, K_MAX = 0.02, 300  # t1 - t0 <= 6: every candidate up to t1 fits below k_max


@pytest.mark.parametrize("G", [5, 32, 48])
def test_march_twin_keeps_the_float64_set_on_generic_rays(G):
    lib = PC.build_host()
    o, d, tr = PC.outside_rays(400, 11 + G)
    n_kept = 0
    for occ in (OC.random_occupancy(G, 7, 0.3), OC.sphere_occupancy(G)):
        res = PC.host_march(lib, o, d, tr, OC.AABB, OC.pack(occ), G, DT, K_MAX)
        tk, cand, keep, clear = PC.ref_march(o, d, tr, occ, G, DT, K_MAX)
        kept = PC.kept_matrix(res, tk, tr, DT)
        assert not (kept & ~cand).any()  # only candidates are kept
        look = cand & clear
        assert np.array_equal(kept[look], keep[look]), int((kept[look] != keep[look]).sum())
        excluded = float((cand & ~clear).sum()) / float(cand.sum())
        print("G = %d: %d candidates, %d kept, share excluded by the face margin %.2e" % (G, cand.sum(), kept.sum(), excluded))
        assert excluded <= 0.01, excluded
        assert not res["overflow"] and res["total"] == kept.sum() == res["count"].sum()
        assert np.array_equal(res["ray_count"], res["count"])
        n_kept += int(kept.sum())
        # the per-sample outputs: the ray's point at t, the unit direction, delta = dt * |d|
        r = res["ray_idx"].astype(np.int64)
        p64 = o[r].astype(np.float64) + res["t"][:, None].astype(np.float64) * d[r]
        assert np.abs(res["xyz"] - p64).max() < 1e-6 * np.abs(p64).max()
        ln = np.linalg.norm(d.astype(np.float64), axis=1)
        assert np.abs(res["dirs"] - (d / ln[:, None])[r]).max() < 1e-6 and np.abs(res["deltas"] / (DT * ln[r]) - 1).max() < 1e-6
    assert n_kept > 1000


@pytest.mark.parametrize("G,k_max", [(5, 200), (32, 64), (48, 1)])
def test_march_twin_invariants_on_special_rays(G, k_max):
    lib = PC.build_host()
    o, d, tr, kinds = OC.rays(5)
    # non-finite inputs and t0 > t1 on top of the special rays of the occupancy tests
    o, d, tr = o.copy(), d.copy(), tr.copy()
    o[0, 1], d[1, 2], tr[2, 0], tr[3, 1] = np.nan, np.inf, np.nan, -np.inf
    tr[4] = (2.0, 1.0)
    dt = 0.05
    for occ in (OC.random_occupancy(G, 7, 0.3), OC.sphere_occupancy(G)):
        bits = OC.pack(occ)
        res = PC.host_march(lib, o, d, tr, OC.AABB, bits, G, dt, k_max)
        cnt, start, total = res["count"], res["ray_start"], res["total"]
        assert total == cnt.sum() and (cnt >= 0).all() and (cnt <= k_max).all() and total > 0
        assert np.array_equal(start, np.cumsum(cnt) - cnt) and np.array_equal(res["ray_count"], cnt) and not res["overflow"]
        assert (cnt[:5] == 0).all()  # non-finite, t0 > t1
        assert (cnt[kinds["miss"]] == 0).all()
        _, hit, _ = OC.host_ray_span(OC.build_host(), o, d, tr, OC.AABB, bits, G)
        assert (cnt[hit == 0] == 0).all()  # a miss keeps nothing
        assert np.array_equal(res["ray_idx"], np.repeat(np.arange(OC.N_RAYS, dtype=np.int32), cnt))
        same_ray = res["ray_idx"][1:] == res["ray_idx"][:-1]
        assert (np.diff(res["t"])[same_ray] > 0).all()  # ascending within a ray
        assert OC.host_mask(OC.build_host(), res["xyz"], OC.AABB, bits, G).all()  # every kept point has its bit set
        tk, cand, _, _ = PC.ref_march(o, d, tr, occ, G, dt, k_max)
        assert not (PC.kept_matrix(res, tk, tr, dt) & ~cand).any()
        # truncation
        last = int(np.nonzero(cnt)[0][-1])
        for cap in (total, total - 1, 0, total + 5):
            cut = PC.host_march(lib, o, d, tr, OC.AABB, bits, G, dt, k_max, cap=cap)
            assert cut["total"] == total and cut["overflow"] == (total > cap)
            n = min(cap, total)
            want = cnt.copy()
            if cap == total - 1:
                want[last] -= 1
            elif cap == 0:
                want[:] = 0
            assert np.array_equal(cut["ray_count"], want) and cut["ray_count"].sum() == n
            for k in ("t", "deltas", "xyz", "dirs", "ray_idx"):
                assert np.array_equal(cut[k][:n].view(np.uint32), res[k][:n].view(np.uint32)), (cap, k)
            # parked rows: outside the box, ray_idx -1, t = delta = 0
            assert (cut["ray_idx"][n:] == -1).all() and (cut["t"][n:] == 0).all() and (cut["deltas"][n:] == 0).all()
            assert not OC.host_mask(OC.build_host(), cut["xyz"][n:], OC.AABB, np.full_like(bits, 0xFFFFFFFF), G).any()
            assert np.isfinite(cut["dirs"]).all()


def test_march_twin_empty_grid_and_no_rays():
    lib = PC.build_host()
    o, d, tr = PC.outside_rays(65, 3)
    G = 5
    res = PC.host_march(lib, o, d, tr, OC.AABB, np.zeros(OC.n_words(G), np.uint32), G, DT, K_MAX, cap=4)
    assert res["total"] == 0 and not res["overflow"] and (res["ray_count"] == 0).all() and (res["ray_idx"] == -1).all()
    res = PC.host_march(lib, o[:0], d[:0], tr[:0], OC.AABB, OC.pack(OC.sphere_occupancy(G)), G, DT, K_MAX, cap=4)
    assert res["total"] == 0 and not res["overflow"] and (res["ray_idx"] == -1).all()


@pytest.mark.parametrize("channels,modes", [((1,), (0,)), ((3,), (0,)), ((4,), (0,)), ((3, 1), (0, 0)), ((3, 4, 1), (0, 1, 2)), ((4, 3, 1), (2, 0, 1)),
                                            ((1, 3, 4), (1, 2, 0))])
def test_composite_twin_matches_the_oracle_in_float64(channels, modes):
    """lengths 0, 1, 2, 63, 64, 65, 129 in one packed list; channels 1, 3, 4 and modes 0, 1, 2 in every position"""
    lib = PC.build_host()
    case = PC.composite_case(channels, modes, seed=sum(channels) * 10 + len(modes))
    ref = PC.ref_composite(case)
    got = PC.host_composite(lib, case["density"], case["deltas"], case["fields"], case["modes"], case["start"], case["count"], case["g_mask"], case["g_out"])
    PC.check_composite(got, ref, "twin %s %s" % (channels, modes))
    assert got["mask"][0] == 0 and (got["out"][0] == 0).all()  # the ray without samples, mode 2 included
    tail = slice(case["P"] - 3, None)  # rows of no ray: never written
    assert (got["g_density"][tail] == 0).all() and all((g[tail] == 0).all() for g in got["g_fields"])
    if 1 in modes:  # detached weights: the mode-1 field's values do not reach the density
        other = dict(case, fields=[f * (3.0 if m == 1 else 1.0) for f, m in zip(case["fields"], modes)])
        got2 = PC.host_composite(lib, other["density"], other["deltas"], other["fields"], modes, case["start"], case["count"], case["g_mask"], case["g_out"])
        assert np.array_equal(got2["g_density"], got["g_density"])


def test_composite_twin_zero_length_ray_between_long_ones():
    lib = PC.build_host()
    case = PC.composite_case((3, 1), (0, 2), seed=5, lengths=(129, 0, 70), gap=0)
    solo = PC.composite_case((3, 1), (0, 2), seed=5, lengths=(129, 70), gap=0)  # the same rows without the empty ray
    a = PC.host_composite(lib, case["density"], case["deltas"], case["fields"], case["modes"], case["start"], case["count"], case["g_mask"], case["g_out"])
    b = PC.host_composite(lib, case["density"], case["deltas"], case["fields"], case["modes"], solo["start"], solo["count"], case["g_mask"][[0, 2]],
                          case["g_out"][[0, 2]])
    assert a["mask"][1] == 0 and (a["out"][1] == 0).all()
    assert np.array_equal(a["mask"][[0, 2]], b["mask"]) and np.array_equal(a["out"][[0, 2]], b["out"]) and np.array_equal(a["g_density"], b["g_density"])
    PC.check_composite(a, PC.ref_composite(case), "twin, empty ray between long ones")


def test_twin_runs_clean_under_the_sanitizers():
    """the stand-alone program over the truncation cases and the rays without samples, AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU"""
    r = subprocess.run([host_twin.sanitized_main("packed")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "packed_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
