"""CPU twin of the importance resampling of a packed list (tests/host_harness/presample/presample_host.cpp over lab4d_amd/csrc/presample_math.hpp)
against the rules of include/lab4d_presample.h restated with numpy (tests/presample_checks.py), its properties, the float64 CDF domain, and
the tie to the reference's sample_pdf.  The GPU suite holds the kernels to this twin (tests/test_gpu_zzzzzzzzzzzzzzpresample.py); here the
twin itself is pinned, with the checks of the library and of lab4d_amd.packed.weights / resample that need no GPU.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import presample_checks as PS  # noqa: E402

f32 = np.float32


@pytest.mark.parametrize("R", PS.RAYS)
def test_twin_equals_the_numpy_rules(R):
    """every output of both calls at n_imp = 1 / 2 / 64 / 65 / 130, with the stratified queries, with a caller's sorted u and with a caller's
    u that is unsorted, partly outside [0, 1] and holds NaN (the ORDER rule's running maximum then decides t), at the capacities
    total, total - 1, a cut in the middle of a ray and 0: cdf, mass, counts, t, deltas, xyz, dirs (by their words), ray_idx, src_row, the
    clamped counts, total, overflow, the parked rows, and the sentinels behind the capacity and in the rows of no ray"""
    lib = PS.build_host()
    case = PS.make_list(R, seed=500 + R)
    for n_imp in PS.N_IMP:
        for u in (None, PS.uniforms(case, n_imp, seed=n_imp), PS.unsorted_uniforms(case, n_imp, seed=n_imp)):
            full = PS.ref_resample(case, n_imp, u)
            live = sum(1 for r in range(R) if PS.rows_of(case, r)[1] > 0)
            assert full["total"] == n_imp * live and (full["cdf"] == PS.SENTINEL_F).sum() == case["P"] - sum(PS.rows_of(case, r)[1] for r in range(R))
            caps = PS.capacities(full)
            assert caps[0] == 0 and caps[-1] == full["total"] and (len(caps) == 4 or n_imp == 1 or live == 1)
            for cap in caps:
                ref, got = PS.under_cap(case, full, cap), PS.host_resample(lib, case, n_imp, u, cap=cap)
                PS.assert_same(got, ref, (R, n_imp, u is not None, cap))
                m = min(cap, full["total"])
                assert got["ray_count"].sum() == m and got["overflow"] == (full["total"] > cap)
                assert (got["src_row"][m:cap] == -1).all() and (got["ray_idx"][m:cap] == -1).all() and (got["t"][m:cap] == 0).all() and (got["deltas"][m:cap] == 0).all()
                for k in PS.OUT_F + PS.OUT_I:  # the rows >= cap are not written
                    assert (got[k][cap:] == (PS.SENTINEL_F if k in PS.OUT_F else PS.SENTINEL_I)).all() and got[k].shape[0] == cap + PS.PAD, (cap, k)


def test_the_test_lists_hold_what_they_promise():
    case = PS.make_list(65, seed=565)
    rows = [PS.rows_of(case, r) for r in range(65)]
    assert set(PS.LENGTHS) <= {n for _, n in rows} and rows[-1][1] == 5 and case["count"][-1] == 65 and case["start"][-2] == -3 and rows[-2] == (0, 0)
    s, n = rows[-3]
    assert n == 65 and (case["weights"][s:s + n] == 0).all()  # the all-zero ray
    owned = np.zeros(case["P"], bool)
    for s, n in rows:
        owned[s:s + n] = True
        t, w = case["t"][s:s + n].astype(np.float64), case["width"][s:s + n].astype(np.float64)
        assert ((t * 64) % 1 == 0).all() and (t > 0).all() and np.isin(w, [1 / 64, 1 / 128]).all()
        assert (t[1:] - w[1:] / 2 >= t[:-1] + w[:-1] / 2).all()  # disjoint intervals, ascending
    w = case["weights"][owned]
    assert (~owned).sum() > 20 and np.isnan(w).sum() >= 5 and (w < 0).sum() >= 5 and (w == 0).sum() > 100
    length = PS.dir_length(case["dir"])
    assert length.min() < 0.6 and length.max() > 1.9
    for r, (s, n) in enumerate(rows):
        assert np.array_equal(case["deltas"][s:s + n], case["width"][s:s + n] * length[r])


@pytest.mark.parametrize("R", [1, 65, 1025])
def test_twin_properties(R):
    """t is non-decreasing per ray; each t_k lies inside the interval of its src_row, up to one rounding; src_row is non-decreasing where
    the prefixes are monotone (and is the row numpy's searchsorted finds there); deltas never exceeds the source row's; with eps = 0 an
    all-zero ray emits nothing"""
    lib = PS.build_host()
    case = PS.make_list(R, seed=900 + R)
    for n_imp in (2, 65, 130):
        ref = PS.ref_resample(case, n_imp)
        got = PS.host_resample(lib, case, n_imp)
        assert np.array_equal(got["ray_idx"][:got["total"]], np.repeat(np.arange(R, dtype=np.int32), got["count"]))
        for r in range(R):
            s, n = PS.rows_of(case, r)
            a, c = int(got["ray_start"][r]), int(got["count"][r])
            assert c == (n_imp if n > 0 else 0)
            if c == 0:
                continue
            t, src = got["t"][a:a + c].astype(np.float64), got["src_row"][a:a + c]
            assert (np.diff(t) >= 0).all() and src.min() >= s and src.max() < s + n, r
            lo = case["t"][src].astype(np.float64) - case["width"][src] / 2
            hi = case["t"][src].astype(np.float64) + case["width"][src] / 2
            slack = 2.0 ** -23 * np.maximum(np.abs(t), 1e-30)  # one rounding of t, and of the width
            assert (t >= lo - slack).all() and (t <= hi + slack).all(), r
            assert (got["deltas"][a:a + c] <= case["deltas"][src]).all() and (got["deltas"][a:a + c] > 0).all(), r
            if ref["monotone"][r]:
                assert (np.diff(src) >= 0).all(), r
                C = got["cdf"][s:s + n]
                q = ((np.arange(n_imp, dtype=f32) + f32(0.5)) / f32(n_imp)) * got["mass"][r]
                assert np.array_equal(src - s, np.minimum(np.searchsorted(C, q, side="right"), n - 1)), r
    zero = PS.host_resample(lib, case, 65, eps=0.0)
    if R >= 3:
        assert zero["count"][R - 3] == 0 and zero["mass"][R - 3] == 0 and PS.host_resample(lib, case, 65)["count"][R - 3] == 65
        assert zero["total"] == 65 * (sum(1 for r in range(R) if PS.rows_of(case, r)[1] > 0 and zero["mass"][r] > 0))


@pytest.mark.parametrize("R", [65, 1025])
def test_order_rule_decides_t_for_an_unsorted_u(R):
    """a caller's u that is unsorted, partly outside [0, 1] and holds NaN, at n_imp = 65 and 130 so that the carry of the running maximum
    crosses the 64-sample chunks: the placed depths t' do decrease within the rays, the twin's t is their running maximum word for word
    (numpy's maximum.accumulate), non-decreasing within every ray, and behind the first chunk rows exist that hold a maximum reached in an
    EARLIER chunk -- what the carry alone provides"""
    lib = PS.build_host()
    case = PS.make_list(R, seed=500 + R)
    for n_imp in (65, 130):
        u = PS.unsorted_uniforms(case, n_imp, seed=n_imp)
        ref, got = PS.ref_resample(case, n_imp, u), PS.host_resample(lib, case, n_imp, u)
        total = ref["total"]
        assert got["total"] == total and np.array_equal(PS.words(got["t"][:total]), PS.words(ref["t"]))
        placed, t = ref["t_placed"].reshape(-1, n_imp), got["t"][:total].reshape(-1, n_imp)
        assert (np.diff(t, axis=1) >= 0).all() and (np.diff(placed, axis=1) < 0).any(axis=1).mean() > 0.9
        assert (t != placed).mean() > 0.5  # without ORDER most words of t would differ
        for c0 in range(64, n_imp, 64):  # rows of a later chunk that still hold the maximum of the chunks before
            carried = (t[:, c0:] == t[:, c0 - 1:c0]) & (placed[:, c0:] < t[:, c0:])
            assert carried.any(axis=1).mean() > 0.5, (n_imp, c0)


@pytest.mark.parametrize("n", [1, 2, 64, 128])
def test_identity_on_equal_weights(n):
    """a ray of n rows of equal weight 2^-3, eps = 0, n_imp = n, u = NULL: its own t and deltas bit for bit, src_row = the row"""
    lib = PS.build_host()
    rng = np.random.default_rng(n)
    d = f32([[0.0, 0.0, 2.0]])
    t = (np.cumsum(rng.integers(1, 3, n)) / 64.0).astype(f32)
    width = rng.choice(f32([1.0 / 64.0, 1.0 / 128.0]), n)
    case = {"R": 1, "P": n, "start": np.zeros(1, np.int32), "count": np.full(1, n, np.int32), "aabb": PS.AABB, "origin": f32([[0.01, 0.02, 0.03]]), "dir": d,
            "t": t, "width": width, "deltas": (width * f32(2.0)).astype(f32), "weights": np.full(n, 0.125, f32)}
    got = PS.host_resample(lib, case, n, eps=0.0)
    assert got["total"] == n and np.array_equal(got["src_row"][:n], np.arange(n))
    assert np.array_equal(PS.words(got["t"][:n]), PS.words(t)) and np.array_equal(PS.words(got["deltas"][:n]), PS.words(case["deltas"]))
    assert np.array_equal(got["dirs"][:n], np.broadcast_to(f32([0, 0, 1]), (n, 3))) and np.array_equal(got["xyz"][:n], case["origin"] + t[:, None] * d)


def test_emitted_depths_in_the_float64_cdf_domain():
    """|F64(t_k) - u_k| <= 1e-4 on the lists above with eps = 1e-5, F64 the float64 piecewise-linear CDF of the same masses: the all-zero
    ray and the near-empty rows included, where comparing t itself would be ill conditioned.  With a caller's unsorted u the emitted t_k is
    the running maximum of the placed depths, so it is held to the running maximum of the clamped u (F64 and its inverse are monotone).
    Measured maximum of the twin: 5.5e-7."""
    lib = PS.build_host()
    worst = 0.0
    for R in (65, 1025):
        case = PS.make_list(R, seed=500 + R)
        for n_imp in PS.N_IMP:
            for u in (None, PS.uniforms(case, n_imp, seed=n_imp), PS.unsorted_uniforms(case, n_imp, seed=n_imp)):
                got = PS.host_resample(lib, case, n_imp, u)
                got["u"] = np.maximum.accumulate(PS.ref_resample(case, n_imp, u)["u"].reshape(-1, n_imp), axis=1).reshape(-1)  # (sorted u: itself)
                err = PS.cdf_errors(case, got)
                worst = max(worst, float(err.max()))
                assert err.max() <= PS.CDF_BAR, (R, n_imp, u is not None, float(err.max()), int(err.argmax()))
    print("cdf domain: max |F64(t_k) - u_k| = %.3e" % worst)


def test_tie_to_the_reference_sample_pdf():
    """rays whose rows tile [near, far], weights >= 0.05, u = linspace(0, 1, n_imp): the emitted depths against oracle.lab4d_oracle.sample_pdf
    on the same bins, both judged in the float64 CDF domain at the 1e-4 bar (and against u itself)"""
    import torch
    from oracle import lab4d_oracle as O
    lib = PS.build_host()
    rng = np.random.default_rng(17)
    R, n, n_imp = 8, 48, 64
    near, far = 0.25, 1.75
    edges = np.sort(np.concatenate([[near, far], near + (far - near) * rng.random(n - 1)])).astype(f32)
    lo, hi = edges[:-1].astype(np.float64), edges[1:].astype(np.float64)
    width = (hi - lo).astype(f32)
    mid = ((lo + hi) / 2).astype(f32)
    d = np.tile(f32([[0.0, 0.0, 1.0]]), (R, 1))
    w = (0.05 + rng.random((R, n))).astype(f32)
    case = {"R": R, "P": R * n, "start": (np.arange(R) * n).astype(np.int32), "count": np.full(R, n, np.int32), "aabb": PS.AABB, "origin": np.zeros((R, 3), f32),
            "dir": d, "t": np.tile(mid, R), "width": np.tile(width, R), "deltas": np.tile(width, R), "weights": w.reshape(-1)}
    u = np.tile(np.linspace(0, 1, n_imp, dtype=f32), (R, 1))
    got = PS.host_resample(lib, case, n_imp, u)
    want = O.sample_pdf(torch.from_numpy(np.tile(edges, (R, 1))), torch.from_numpy(w), n_imp, eps=PS.EPS).numpy()
    assert got["total"] == R * n_imp
    worst = 0.0
    for r in range(R):
        m = w[r].astype(np.float64) + np.float64(f32(PS.EPS))
        mine, ref = PS.cdf64(lo, hi, m, got["t"][r * n_imp:(r + 1) * n_imp]), PS.cdf64(lo, hi, m, want[r])
        worst = max(worst, np.abs(mine - ref).max(), np.abs(mine - u[r]).max())
    print("sample_pdf tie: max CDF-domain difference = %.3e" % worst)
    assert worst <= PS.CDF_BAR and abs(float(got["t"][0]) - near) < 1e-6 and abs(float(got["t"][n_imp - 1]) - far) < 1e-6


def test_weights_twin_against_float64():
    """presample_host_weights (the host's expf) against the float64 compute_weights per ray, at the fp32 bar; a NaN, a negative and an
    infinite density count as tau = 0 / saturate; the rows of no ray keep their sentinel; an empty ray is transparent"""
    lib = PS.build_host()
    case = PS.make_list(65, seed=3)
    rng = np.random.default_rng(4)
    density = (rng.random(case["P"]) * 40).astype(f32)
    s3, _ = PS.rows_of(case, 3)
    density[s3 + 1], density[s3 + 2] = np.nan, -3.0
    w, trans = PS.host_weights(lib, density, case["deltas"], case["start"], case["count"], case["P"])
    owned = np.zeros(case["P"], bool)
    for r in range(65):
        s, n = PS.rows_of(case, r)
        owned[s:s + n] = True
        with np.errstate(invalid="ignore"):
            tau = density[s:s + n].astype(np.float64) * case["deltas"][s:s + n].astype(np.float64)
        tau = np.where(tau > 0, tau, 0.0)
        E = np.cumsum(tau) - tau
        assert np.abs(w[s:s + n] - (1 - np.exp(-tau)) * np.exp(-E)).max(initial=0) <= 1e-4 and abs(trans[r] - np.exp(-tau.sum())) <= 1e-4, r
    assert (w[~owned] == PS.SENTINEL_F).all() and trans[-2] == 1 and w[s3 + 1] == 0 and w[s3 + 2] == 0


def test_sanitized_standalone_program():
    """tests/host_harness/presample_host_main.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, as a child process with its own main:
    unsorted u, NaN / negative / infinite weights, a (start, count) outside [0, P), |dir| = 0; exact-size heap buffers"""
    r = subprocess.run([host_twin.sanitized_main("presample")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "presample_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


def test_call_sites_and_prototypes_of_the_three_entry_points():
    """the entry points are declared with a stream, their signatures are the pinned ones, lab4d_amd/packed.py calls each with as many
    arguments as the prototype has in front of its stream, and the twin's definitions take the same parameters, stream aside"""
    import ast
    import ctypes
    from lab4d_amd import _lib
    vp, cl, ci, cf = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
    pinned = {"lab4d_packed_weights": (ci, [vp] * 4 + [cl, cl, vp, vp, vp], True),
              "lab4d_packed_resample_count": (ci, [vp] * 3 + [cl, cl, ci, cf] + [vp] * 4, True),
              "lab4d_packed_resample_write": (ci, [vp] * 8 + [cl, cl] + [vp] * 3 + [ci, cf, cl] + [vp] * 11, True)}
    for name, want in pinned.items():
        restype, params, has_stream = _lib.SIGNATURES[name]
        assert (restype, _lib.argtypes(params), has_stream) == want, name
    sites = {}
    for node in ast.walk(ast.parse(open(os.path.join(_lib.HERE, "packed.py")).read())):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call" and isinstance(node.func.value, ast.Name)
                and node.func.value.id == "_lib" and isinstance(node.args[0], ast.Constant) and node.args[0].value in ("packed_weights", "packed_resample_count", "packed_resample_write")):
            assert not any(isinstance(a, ast.Starred) for a in node.args)
            sites.setdefault(node.args[0].value, []).append(len(node.args) - 1)
    assert sites == {"packed_weights": [8], "packed_resample_count": [10], "packed_resample_write": [26]}, sites
    with open(os.path.join(host_twin.HARNESS, PS.TWIN + "_host.cpp")) as fh:
        text = fh.read()
    twin = host_twin.signatures(text, PS.TWIN + "_host.cpp")
    assert sorted(twin) == ["presample_host_count", "presample_host_weights", "presample_host_write"] and text.count('extern "C"') == 3
    lib = PS.build_host()
    for mine, theirs in (("weights", "lab4d_packed_weights"), ("count", "lab4d_packed_resample_count"), ("write", "lab4d_packed_resample_write")):
        assert twin["presample_host_" + mine][1] == _lib.argtypes(_lib.SIGNATURES[theirs][1])[:-1], mine
        assert list(getattr(lib, "presample_host_" + mine).argtypes) == twin["presample_host_" + mine][1] and getattr(lib, "presample_host_" + mine).restype is None


def test_library_checks_its_arguments_before_any_launch():
    """argument validation happens before any launch, so it runs without a GPU (tests/test_abi.py builds the library the same way)"""
    import ctypes
    from lab4d_amd import _lib
    _lib.build(verbose=False)
    so = ctypes.CDLL(_lib.SO_PATH)
    so.lab4d_last_error.restype = ctypes.c_char_p
    for name in ("weights", "resample_count", "resample_write"):
        fn = getattr(so, "lab4d_packed_" + name)
        fn.restype, fn.argtypes = ctypes.c_int, _lib.argtypes(_lib.SIGNATURES["lab4d_packed_" + name][1])
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    for R, P, word in ((-1, 4, b"R = -1"), (1 << 31, 4, b"R = "), (1, -1, b"P = -1"), (1, 1 << 31, b"P = ")):
        assert so.lab4d_packed_weights(buf, buf, buf, buf, R, P, buf, buf, None) == -1 and word in so.lab4d_last_error(), (word, so.lab4d_last_error())
    assert so.lab4d_packed_weights(buf, buf, None, None, 1, 4, buf, buf, None) == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_packed_weights(buf, buf, buf, buf, 1, 4, None, buf, None) == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_packed_weights(None, None, None, None, 0, 4, None, None, None) == 0  # no rays: nothing to launch
    bad = ((-1, 4, 8, 1e-5, b"R = -1"), (1, 1 << 31, 8, 1e-5, b"P = "), (1, 4, 0, 1e-5, b"n_imp = 0"), (1 << 20, 4, 1 << 11, 1e-5, b"R * n_imp"),
           (1, 4, 8, -1e-5, b"eps"), (1, 4, 8, float("nan"), b"eps"), (1, 4, 8, float("inf"), b"eps"))
    for R, P, n_imp, eps, word in bad:
        assert so.lab4d_packed_resample_count(buf, buf, buf, R, P, n_imp, eps, buf, buf, buf, None) == -1 and word in so.lab4d_last_error(), (word, so.lab4d_last_error())
    assert so.lab4d_packed_resample_count(buf, buf, buf, 1, 4, 8, 1e-5, buf, None, buf, None) == -1 and b"null" in so.lab4d_last_error()
    assert so.lab4d_packed_resample_count(None, None, None, 0, 4, 8, 0.0, None, None, None, None) == 0  # no rays: nothing to launch

    def write(R, P, n_imp, eps, cap, total=buf, origin=buf):
        return so.lab4d_packed_resample_write(buf, buf, buf, buf, buf, buf, buf, buf, R, P, origin, buf, None, n_imp, eps, cap, buf, buf, buf, buf, buf, buf, buf, buf,
                                              total, buf, None)
    for R, P, n_imp, eps, word in bad:
        assert write(R, P, n_imp, eps, 4) == -1 and word in so.lab4d_last_error(), (word, so.lab4d_last_error())
    for cap in (-1, 1 << 31):
        assert write(1, 4, 8, 1e-5, cap) == -1 and b"cap" in so.lab4d_last_error()
    assert write(1, 4, 8, 1e-5, 4, total=None) == -1 and b"null" in so.lab4d_last_error()
    assert write(1, 4, 8, 1e-5, 4, origin=None) == -1 and b"null" in so.lab4d_last_error()


class _List:
    def __init__(self, P=6, R=2, **kw):
        import torch
        self.t, self.deltas = torch.zeros(P), torch.zeros(P)
        self.ray_start, self.ray_count = torch.zeros(R, dtype=torch.int32), torch.zeros(R, dtype=torch.int32)
        self.cap = P
        for k, v in kw.items():
            setattr(self, k, v)


def test_python_layer_checks_that_need_no_gpu():
    import inspect
    import torch
    from lab4d_amd import hashfield, packed
    z = torch.zeros
    good = dict(weights=z(6), origin=z(2, 3), dir=z(2, 3), n_imp=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.resample(_List(), aabb=z(6), **good)
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.weights(z(6), z(6), _List())
    cases = ((dict(rays=_List(t=z(6, dtype=torch.float64))), r"rays\.t must be float32"), (dict(rays=_List(deltas=z(6, 1))), r"rays\.deltas must be float32"),
             (dict(rays=_List(deltas=z(5))), "disagree on the number of rows"), (dict(rays=_List(ray_start=z(2, dtype=torch.int64))), "must be int32"),
             (dict(weights=z(5)), "weights must be float32"), (dict(weights=z(6, dtype=torch.float16)), "weights must be float32"),
             (dict(origin=z(3, 3)), "disagree with the list's 2 rays"), (dict(dir=z(2, 2)), r"dir must be float32 \(n, 3\)"), (dict(n_imp=0), "n_imp = 0"),
             (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(u=z(2, 5)), r"u must be float32 \(2, 4\)"),
             (dict(u=z(2, 4, dtype=torch.float64)), "u must be float32"), (dict(cap=-1), r"cap = -1 outside \[0, 2\^31\)"), (dict(cap=1 << 31), "cap = "),
             (dict(aabb=z(5)), "aabb must be float32"), (dict(n_imp=1 << 30), "does not fit 31 bits"))
    for kw, word in cases:
        args = dict(good, rays=_List(), aabb=z(6))
        args.update(kw)
        rays, weights, origin, dir, n_imp = (args.pop(k) for k in ("rays", "weights", "origin", "dir", "n_imp"))
        with pytest.raises(RuntimeError, match=word):
            packed.resample(rays, weights, origin, dir, n_imp, **args)
    for kw, word in ((dict(density=z(6, dtype=torch.float16)), "density must be float32"), (dict(density=z(6, 1, 1)), "density must be float32"),
                     (dict(deltas=z(5)), "deltas must be float32"), (dict(deltas=z(6, dtype=torch.float64)), "deltas must be float32"),
                     (dict(rays=_List(ray_count=z(3, dtype=torch.int32))), "must be int32")):
        args = dict(density=z(6), deltas=z(6), rays=_List())
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            packed.weights(**args)
    sig = inspect.signature(packed.resample)
    assert list(sig.parameters) == ["rays", "weights", "origin", "dir", "n_imp", "aabb", "u", "eps", "cap"] and sig.parameters["eps"].default == 1e-5
    assert sig.parameters["aabb"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["cap"].default is None
    sig = inspect.signature(hashfield.render_packed_resampled)
    assert list(sig.parameters)[:12] == ["P", "cfg", "grid", "origin", "dir", "t_range", "dt", "cap", "n_imp", "fine_cap", "u", "eps"]


def test_kernels_have_no_private_segment_and_no_spills(tmp_path):
    kernels = host_twin.kernel_metadata("presample.hip", tmp_path)
    names = [k["name"] for k in kernels]
    want = ("k_packed_weights", "k_packed_resample_count", "k_packed_resample_write", "k_packed_resample_park")
    assert len(names) == 4 and all(any(n in x for x in names) for n in want), names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "agpr_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
    assert max(k["vgpr_count"] for k in kernels) <= 64, kernels  # eight waves per SIMD by the vector registers
