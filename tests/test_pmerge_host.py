"""CPU twin of the merge of two packed lists (tests/host_harness/pmerge/pmerge_host.cpp over lab4d_amd/csrc/pmerge_math.hpp) against the rules of
include/lab4d_pmerge.h restated with numpy's stable argsort (tests/pmerge_checks.py).  The GPU suite holds the kernels to this twin
(tests/test_gpu_zzzzzzzzzzzzzpmerge.py); here the twin itself is pinned, with the checks of lab4d_amd.packed.merge / merge_rows that need no
GPU.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import pmerge_checks as PM  # noqa: E402


@pytest.mark.parametrize("R", [1, 63, 64, 65, 1025])
def test_twin_equals_the_stable_argsort(R):
    """every output of both calls at the capacities total, total - 1, a cut in the middle of a ray and 0: src and from it pos_a, pos_b, t,
    deltas (by their words), ray_idx, the clamped counts, total, overflow, -1 in pos behind the cut, the parked rows, and the sentinel in
    the PAD rows behind the capacity"""
    lib = PM.build_host()
    case = PM.make_pair(R, seed=300 + R)
    full = PM.ref_merge(case)
    owned = sum(PM.rows_of(case, w, r)[1] for w in "ab" for r in range(R))
    assert full["total"] == owned == full["count"].sum() and not full["overflow"]
    caps = PM.capacities(case, full["total"], full["count"], full["ray_start"])
    assert len(caps) == 4 and caps[0] == 0 and caps[-1] == full["total"]
    for cap in caps:
        ref, got = PM.ref_merge(case, cap), PM.host_merge(lib, case, cap)
        PM.assert_same(got, ref, (R, cap))
        m = min(cap, full["total"])
        assert got["ray_count"].sum() == m and got["overflow"] == (full["total"] > cap)
        assert (got["pos_a"] >= 0).sum() + (got["pos_b"] >= 0).sum() == m and max(got["pos_a"].max(), got["pos_b"].max()) < max(cap, 1)
        assert (got["src"][m:cap] == -1).all() and (got["ray_idx"][m:cap] == -1).all() and (got["t"][m:cap] == 0).all() and (got["deltas"][m:cap] == 0).all()
        for k in PM.MERGED_F + PM.MERGED_I:  # the rows >= cap are not written
            assert (got[k][cap:] == (PM.SENTINEL_F if k in PM.MERGED_F else PM.SENTINEL_I)).all() and got[k].shape[0] == cap + PM.PAD, (cap, k)


def test_the_test_lists_hold_what_they_promise():
    case = PM.make_pair(65, seed=365)
    rows = [(PM.rows_of(case, "a", r)[1], PM.rows_of(case, "b", r)[1]) for r in range(65)]
    kind = lambda n: 0 if n == 0 else (1 if n < 64 else 2)
    assert {(kind(a), kind(b)) for a, b in rows} == {(i, j) for i in range(3) for j in range(3)}
    assert {64, 65, 127, 128, 129} <= {a + b for a, b in rows}
    assert rows[-1] == (5, 3) and case["count_a"][-1] == 65 and case["count_b"][-1] == 40 and case["start_a"][-4] == -3 and rows[-4] == (0, 2)
    (sa, ma), (sb, mb) = PM.rows_of(case, "a", 63), PM.rows_of(case, "b", 63)
    assert ma == mb == 65 and np.array_equal(PM.words(case["t_a"][sa:sa + ma]), PM.words(case["t_b"][sb:sb + mb]))  # the same values in both lists
    (sa, ma), (sb, mb) = PM.rows_of(case, "a", 62), PM.rows_of(case, "b", 62)
    assert (ma, mb) == (64, 63) and case["t_a"][sa:sa + ma].min() > case["t_b"][sb:sb + mb].max()  # all of A behind all of B
    ties = gaps = 0
    for r in range(65):
        (sa, ma), (sb, mb) = PM.rows_of(case, "a", r), PM.rows_of(case, "b", r)
        ta, tb = case["t_a"][sa:sa + ma], case["t_b"][sb:sb + mb]
        assert (np.diff(ta) >= 0).all() and (np.diff(tb) >= 0).all()
        ties += len(np.intersect1d(ta, tb))
    for w in "ab":
        owned = np.zeros(case["P" + w], bool)
        for r in range(65):
            s, n = PM.rows_of(case, w, r)
            owned[s:s + n] = True
        gaps += int((~owned).sum())
    both = np.concatenate([case["t_a"], case["t_b"]])
    assert ties > 500 and gaps > 20 and np.signbit(both[both == 0]).any() and not np.signbit(both[both == 0]).all()


@pytest.mark.parametrize("R", [1, 65, 1025])
def test_twin_properties(R):
    """src restricted to a ray is a permutation of its rows, src[pos_a[i]] == i, src[pos_b[i]] == Pa + i, the merged t is non-decreasing
    within every ray, a tie between the lists goes to A and the order inside a list is kept"""
    lib = PM.build_host()
    case = PM.make_pair(R, seed=900 + R)
    got = PM.host_merge(lib, case)
    Pa, src, total = case["Pa"], got["src"], got["total"]
    assert np.array_equal(got["ray_start"], np.cumsum(got["count"]) - got["count"]) and np.array_equal(got["ray_count"], got["count"])
    assert np.array_equal(got["ray_idx"][:total], np.repeat(np.arange(R, dtype=np.int32), got["count"]))
    cat_t, cat_d = np.concatenate([case["t_a"], case["t_b"]]), np.concatenate([case["deltas_a"], case["deltas_b"]])
    assert np.array_equal(PM.words(got["t"][:total]), PM.words(cat_t[src[:total]])) and np.array_equal(PM.words(got["deltas"][:total]), PM.words(cat_d[src[:total]]))
    tie_pairs = 0
    for r in range(R):
        (sa, ma), (sb, mb) = PM.rows_of(case, "a", r), PM.rows_of(case, "b", r)
        s0 = int(got["ray_start"][r])
        mine, t = src[s0:s0 + ma + mb], got["t"][s0:s0 + ma + mb]
        assert np.array_equal(np.sort(mine), np.concatenate([np.arange(sa, sa + ma), Pa + np.arange(sb, sb + mb)])), r
        assert (np.diff(t) >= 0).all(), r
        assert (np.diff(mine[mine < Pa]) > 0).all() and (np.diff(mine[mine >= Pa]) > 0).all(), r  # the order inside a list is kept
        tied = t[1:] == t[:-1]
        assert not (tied & (mine[:-1] >= Pa) & (mine[1:] < Pa)).any(), r  # never B in front of A at the same t
        tie_pairs += int((tied & (mine[:-1] < Pa) & (mine[1:] >= Pa)).sum())
    owned_a, owned_b = got["pos_a"] >= 0, got["pos_b"] >= 0
    assert np.array_equal(src[got["pos_a"][owned_a]], np.flatnonzero(owned_a)) and np.array_equal(src[got["pos_b"][owned_b]], Pa + np.flatnonzero(owned_b))
    assert owned_a.sum() + owned_b.sum() == total and (R < 65 or tie_pairs > 100)


def test_merging_with_an_empty_list_is_the_identity():
    lib = PM.build_host()
    case = PM.make_pair(65, seed=4, gaps=False)
    for keep, drop in ("ab", "ba"):
        one = dict(case)
        one["count_" + drop] = np.zeros_like(case["count_" + drop])
        got = PM.host_merge(lib, one)
        n = sum(PM.rows_of(case, keep, r)[1] for r in range(65))
        s, m = PM.rows_of(case, keep, 64)
        assert got["total"] == n and (got["pos_" + drop] == -1).all()
        assert np.array_equal(got["src"][:n] - (case["Pa"] if keep == "b" else 0), np.arange(n)) and s + m == n == case["P" + keep]  # (no gaps)
        assert np.array_equal(PM.words(got["t"][:n]), PM.words(case["t_" + keep])) and np.array_equal(PM.words(got["deltas"][:n]), PM.words(case["deltas_" + keep]))


def test_no_rays_and_no_rows():
    lib = PM.build_host()
    got = PM.host_merge(lib, PM.make_pair(0, seed=1), cap=3)
    assert got["total"] == 0 and not got["overflow"] and (got["src"][:3] == -1).all() and (got["ray_idx"][:3] == -1).all() and (got["t"][:3] == 0).all()
    case = PM.make_pair(5, seed=1)
    for k in ("t_a", "deltas_a", "t_b", "deltas_b"):
        case[k] = case[k][:0]
    case["Pa"] = case["Pb"] = 0
    got = PM.host_merge(lib, case, cap=3)
    assert got["total"] == 0 and (got["ray_count"] == 0).all() and (got["src"][:3] == -1).all() and (got["src"][3:] == PM.SENTINEL_I).all()


def test_unsorted_and_nan_input_stays_inside_its_ray():
    """the two guarantees for input that breaks the precondition: the call returns, and every row it wrote lies inside its ray's merged rows
    (ray_idx of a written row is the ray that owns the row; the rows behind the capacity keep their sentinel)"""
    lib = PM.build_host()
    case = PM.make_pair(65, seed=12)
    rng = np.random.default_rng(3)
    for w in "ab":
        t = rng.standard_normal(case["P" + w]).astype(np.float32)
        t[rng.random(t.shape[0]) < 0.2] = np.nan
        case["t_" + w] = t
    full = PM.host_merge(lib, case)
    for cap in (full["total"], full["total"] // 2):
        got = PM.host_merge(lib, case, cap)
        want = np.repeat(np.arange(65, dtype=np.int32), full["count"])[:cap]
        written = got["ray_idx"][:cap] != PM.SENTINEL_I
        assert np.array_equal(got["ray_idx"][:cap][written], want[written]) and (got["src"][cap:] == PM.SENTINEL_I).all()


@pytest.mark.parametrize("C", [1, 3, 64])
def test_gather_twin_and_its_adjoint(C):
    """both parts, a NULL part, idx = -1 and idx behind both parts; the adjoint through pos equals the transpose of the forward on random
    g_out bit for bit, since every value is a copy"""
    lib = PM.build_host()
    case = PM.make_pair(65, seed=77)
    Pa, Pb = case["Pa"], case["Pb"]
    rng = np.random.default_rng(C)
    a, b = rng.standard_normal((Pa, C)).astype(np.float32), rng.standard_normal((Pb, C)).astype(np.float32)
    total = PM.host_merge(lib, case)["total"]
    got = PM.host_merge(lib, case, cap=total - 40, pad=0)  # (rows fall behind the capacity: their pos is -1)
    cap, src = got["cap"], got["src"]
    assert (src >= 0).all() and (got["pos_a"] == -1).any()
    cat = np.concatenate([a, b])
    out = PM.host_gather(lib, a, Pa, b, Pb, src, C)
    assert np.array_equal(PM.words(out), PM.words(cat[src]))
    only_a, only_b = PM.host_gather(lib, a, Pa, None, Pb, src, C), PM.host_gather(lib, None, Pa, b, Pb, src, C)
    assert np.array_equal(PM.words(only_a), PM.words(np.where((src < Pa)[:, None], out, np.float32(0))))
    assert np.array_equal(PM.words(only_b), PM.words(np.where((src >= Pa)[:, None], out, np.float32(0))))
    odd = np.array([-1, 0, Pa - 1, Pa, Pa + Pb - 1, Pa + Pb, 2 ** 31 - 1, -2 ** 31], np.int32)
    want = np.stack([np.zeros(C, np.float32), a[0], a[-1], b[0], b[-1], np.zeros(C, np.float32), np.zeros(C, np.float32), np.zeros(C, np.float32)])
    assert np.array_equal(PM.words(PM.host_gather(lib, a, Pa, b, Pb, odd, C)), PM.words(want))
    # the adjoint: g_a[i] = g_out[pos_a[i]] (0 where pos_a[i] = -1) is the transpose of out = a[src]
    g_out = rng.standard_normal((cap, C)).astype(np.float32)
    g_a, g_b = PM.host_gather(lib, g_out, cap, None, 0, got["pos_a"], C), PM.host_gather(lib, g_out, cap, None, 0, got["pos_b"], C)
    want_a, want_b = np.zeros((Pa, C), np.float32), np.zeros((Pb, C), np.float32)
    np.add.at(want_a, src[src < Pa], g_out[src < Pa])
    np.add.at(want_b, src[src >= Pa] - Pa, g_out[src >= Pa])
    assert np.array_equal(PM.words(g_a), PM.words(want_a)) and np.array_equal(PM.words(g_b), PM.words(want_b))


def test_call_sites_and_prototypes_of_the_three_entry_points():
    """the ABI walk of tests/test_abi.py for the new launch sites: the entry points are declared with a stream, their signatures are the
    pinned ones, lab4d_amd/packed.py calls each with as many arguments as the prototype has in front of its stream, and the twin's
    definitions take the same parameters, stream aside"""
    import ast
    import ctypes
    from lab4d_amd import _lib
    vp, cl, ci = ctypes.c_void_p, ctypes.c_long, ctypes.c_int
    pinned = {"lab4d_packed_merge_count": (ci, [vp, vp, cl, vp, vp, cl, cl, vp, vp], True),
              "lab4d_packed_merge_write": (ci, [vp] * 4 + [cl] + [vp] * 4 + [cl, cl, vp, cl] + [vp] * 10, True),
              "lab4d_packed_merge_gather": (ci, [vp, cl, vp, cl, vp, cl, ci, vp, vp], True)}
    for name, want in pinned.items():
        restype, params, has_stream = _lib.SIGNATURES[name]
        assert (restype, _lib.argtypes(params), has_stream) == want, name
    sites = {}
    for node in ast.walk(ast.parse(open(os.path.join(_lib.HERE, "packed.py")).read())):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call" and isinstance(node.func.value, ast.Name)
                and node.func.value.id == "_lib" and isinstance(node.args[0], ast.Constant) and node.args[0].value.startswith("packed_merge_")):
            assert not any(isinstance(a, ast.Starred) for a in node.args)
            sites.setdefault(node.args[0].value, []).append(len(node.args) - 1)
    assert sites == {"packed_merge_count": [8], "packed_merge_write": [22], "packed_merge_gather": [8, 8]}, sites
    with open(os.path.join(host_twin.HARNESS, PM.TWIN + "_host.cpp")) as fh:
        text = fh.read()
    twin = host_twin.signatures(text, PM.TWIN + "_host.cpp")
    assert sorted(twin) == ["pmerge_host_count", "pmerge_host_gather", "pmerge_host_write"] and text.count('extern "C"') == 3  # (every function of the twin is typed)
    lib = PM.build_host()
    for name in ("count", "write", "gather"):
        assert twin["pmerge_host_" + name][1] == _lib.argtypes(_lib.SIGNATURES["lab4d_packed_merge_" + name][1])[:-1], name
        assert list(getattr(lib, "pmerge_host_" + name).argtypes) == twin["pmerge_host_" + name][1] and getattr(lib, "pmerge_host_" + name).restype is None


def test_library_checks_its_arguments_before_any_launch():
    """argument validation happens before any launch, so it runs without a GPU (tests/test_abi.py builds the library the same way)"""
    import ctypes
    from lab4d_amd import _lib
    _lib.build(verbose=False)
    so = ctypes.CDLL(_lib.SO_PATH)
    so.lab4d_last_error.restype = ctypes.c_char_p
    for name in ("count", "write", "gather"):
        fn = getattr(so, "lab4d_packed_merge_" + name)
        fn.restype, fn.argtypes = ctypes.c_int, _lib.argtypes(_lib.SIGNATURES["lab4d_packed_merge_" + name][1])
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    big = 1 << 30
    for Pa, Pb, R, word in ((big, big, 1, b"Pa + Pb"), (-1, 4, 1, b"Pa + Pb"), (4, 4, -1, b"R = -1"), (4, 4, 1 << 31, b"R = ")):
        assert so.lab4d_packed_merge_count(buf, buf, Pa, buf, buf, Pb, R, buf, None) == -1 and word in so.lab4d_last_error(), (word, so.lab4d_last_error())
    assert so.lab4d_packed_merge_count(None, None, 4, None, None, 4, 1, None, None) == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_packed_merge_count(None, None, 4, None, None, 4, 0, None, None) == 0  # no rays: nothing to launch

    def write(Pa, Pb, R, cap, total=buf):
        return so.lab4d_packed_merge_write(buf, buf, buf, buf, Pa, buf, buf, buf, buf, Pb, R, buf, cap, buf, buf, buf, buf, buf, buf, buf, total, buf, None)
    for args, word in (((4, 4, 1, -1), b"cap"), ((4, 4, 1, 1 << 31), b"cap"), ((big, big, 1, 4), b"Pa + Pb"), ((4, 4, -1, 4), b"R = -1"), ((4, 4, 1, 4, None), b"null")):
        assert write(*args) == -1 and word in so.lab4d_last_error(), (word, so.lab4d_last_error())
    for args, word in (((4, 4, 4, 0), b"C = 0"), ((4, 4, 4, 65), b"C = 65"), ((big, big, 4, 3), b"Pa + Pb"), ((4, 4, -1, 3), b"n = -1"), ((4, 4, 1 << 31, 3), b"n = ")):
        Pa, Pb, n, C = args
        assert so.lab4d_packed_merge_gather(buf, Pa, buf, Pb, buf, n, C, buf, None) == -1 and word in so.lab4d_last_error(), (word, so.lab4d_last_error())
    assert so.lab4d_packed_merge_gather(buf, 4, buf, 4, None, 4, 3, buf, None) == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_packed_merge_gather(None, 4, None, 4, None, 0, 3, None, None) == 0  # no rows: nothing to launch


class _List:
    def __init__(self, P=6, R=2, **kw):
        import torch
        self.t, self.deltas = torch.zeros(P), torch.zeros(P)
        self.ray_start, self.ray_count = torch.zeros(R, dtype=torch.int32), torch.zeros(R, dtype=torch.int32)
        self.cap = P
        for k, v in kw.items():
            setattr(self, k, v)


def test_python_layer_checks_that_need_no_gpu():
    import torch
    from lab4d_amd import packed
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.merge(_List(), _List())
    for bad, word in ((dict(t=torch.zeros(6, dtype=torch.float64)), r"rays_a\.t must be float32"), (dict(t=torch.zeros(6, 1)), r"rays_a\.t must be float32"),
                      (dict(deltas=torch.zeros(6, dtype=torch.float16)), r"rays_a\.deltas must be float32"), (dict(deltas=torch.zeros(5)), "disagree on the number of rows"),
                      (dict(ray_start=torch.zeros(2, dtype=torch.int64)), "must be int32"), (dict(ray_count=torch.zeros(3, dtype=torch.int32)), "must be int32")):
        with pytest.raises(RuntimeError, match=word):
            packed.merge(_List(**bad), _List())
    with pytest.raises(RuntimeError, match=r"rays_b\.t must be float32"):
        packed.merge(_List(), _List(t=torch.zeros(6, dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="disagree on the number of rays: 2 and 3"):
        packed.merge(_List(), _List(R=3))
    for cap in (-1, 1 << 31):
        with pytest.raises(RuntimeError, match=r"cap = -?\d+ outside \[0, 2\^31\)"):
            packed.merge(_List(), _List(), cap=cap)
    huge = torch.empty(1 << 30, device="meta")  # (no storage: only its shape is looked at before the check fires)
    with pytest.raises(RuntimeError, match="does not fit 31 bits"):
        packed.merge(_List(t=huge, deltas=huge), _List(t=huge, deltas=huge))
    merged = packed.MergedRays(t=None, deltas=None, ray_idx=None, src=torch.tensor([0, 7, -1], dtype=torch.int32), pos_a=torch.zeros(6, dtype=torch.int32),
                               pos_b=torch.zeros(4, dtype=torch.int32), ray_start=None, ray_count=None, total=None, overflow=None, R=2, cap=3, Pa=6, Pb=4)
    assert merged.from_b.tolist() == [False, True, False]
    assert packed.MergedRays.__slots__ == ("t", "deltas", "ray_idx", "src", "pos_a", "pos_b", "ray_start", "ray_count", "total", "overflow", "R", "cap", "Pa", "Pb")
    with pytest.raises(RuntimeError, match="both None"):
        packed.merge_rows(merged)
    for kw, word in ((dict(a=torch.zeros(5, 3)), "a must be float32"), (dict(a=torch.zeros(6, 3, dtype=torch.float64)), "a must be float32"),
                     (dict(a=torch.zeros(6, 3), b=torch.zeros(4, 2)), "b must be float32"), (dict(a=torch.zeros(6), b=torch.zeros(4, 1)), "b must be float32"),
                     (dict(b=torch.zeros(4, 1, 1)), "b must be float32"), (dict(a=torch.zeros(6, 65)), "65 channels"), (dict(b=torch.zeros(4, 0)), "0 channels")):
        with pytest.raises(RuntimeError, match=word):
            packed.merge_rows(merged, **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.merge_rows(merged, a=torch.zeros(6, 3))
    from lab4d_amd import hashfield
    assert hashfield.PackedField._fields == ("P", "cfg", "grid", "origin", "dir", "t_range", "dt", "cap")
    assert hashfield.PairRender._fields == ("rgb", "mask", "depth", "mask_a", "mask_b", "total_a", "overflow_a", "total_b", "overflow_b", "total", "overflow")


def test_kernels_have_no_private_segment_and_no_spills(tmp_path):
    kernels = host_twin.kernel_metadata("pmerge.hip", tmp_path)
    names = [k["name"] for k in kernels]
    want = ("k_packed_merge_count", "k_packed_merge_clear", "k_packed_merge_write", "k_packed_merge_park", "k_packed_merge_gather")
    assert len(names) == 5 and all(any(n in x for x in names) for n in want), names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "agpr_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
    assert max(k["vgpr_count"] for k in kernels) <= 64, kernels  # eight waves per SIMD
