"""CPU twin of the proposal loss between two packed lists (tests/host_harness/proposal/proposal_host.cpp over lab4d_amd/csrc/proposal_math.hpp)
against the rules of include/lab4d_proposal.h restated with numpy (tests/proposal_checks.py), its properties, and the float64 brute force;
the twin of the weights adjoint against float64 autograd.  The GPU suite holds the kernels to this twin
(tests/test_gpu_zzzzzzzzzzzzzzzproposal.py); here the twin itself is pinned, with the checks of the library and of
lab4d_amd.packed.render_weights / proposal_loss that need no GPU.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402
import proposal_checks as PR  # noqa: E402

f32 = np.float32


@pytest.mark.parametrize("R", PR.RAYS)
def test_twin_equals_the_numpy_rules(R):
    """every output of the three calls by its words, with eps = the fp32 epsilon and eps = 0: lo_e, hi_e, cdf_e, span, coef, loss, g_w_e; the
    sentinels in the rows of no ray are untouched"""
    lib = PR.build_host()
    case = PR.make_case(R, seed=700 + R)
    for eps in (PR.EPS, 0.0):
        got, ref = PR.host_loss(lib, case, eps), PR.ref_loss(case, eps)
        PR.assert_same(got, ref, (R, eps))
        for key, lst, names in (("e", case["e"], ("lo_e", "hi_e", "cdf_e", "g_w_e")), ("f", case["f"], ("coef",))):
            free = ~PR.owned(lst, R)
            assert (R == 1 or free.sum() >= 5) and all((got[k][free] == PR.SENTINEL_F).all() and not (got[k][~free] == PR.SENTINEL_F).any() for k in names), key
        free = ~PR.owned(case["f"], R)
        assert (got["span"][free] == PR.SENTINEL_I).all() and (got["span"][~free] >= 0).all()


def test_the_test_lists_hold_what_they_promise():
    case = PR.make_case(1025, seed=1725)
    e, f, R = case["e"], case["f"], 1025
    pairs = {(PR.rows_of(e, r)[1], PR.rows_of(f, r)[1]) for r in range(R)}
    assert {(a, b) for a in PR.LENGTHS for b in PR.LENGTHS} <= pairs and (0, 200) in pairs and (200, 0) in pairs
    assert PR.rows_of(e, R - 1) == (e["P"] - 5, 5) and PR.rows_of(f, R - 1) == (f["P"] - 5, 5) and e["count"][-1] == 65  # leaves [0, P): cut
    assert PR.rows_of(e, R - 2) == (0, 0) and e["start"][-2] == -3 and f["start"][-2] == -3
    length = PR.dir_length(case["dir"])
    assert length[R - 3] == 0 and PR.rows_of(e, R - 3)[1] == 65 and PR.rows_of(f, R - 3)[1] == 65
    assert (length > 0).sum() == R - 1 and length[length > 0].min() < 0.6 and length.max() > 1.9
    assert (~PR.owned(e, R)).sum() > 20 and (~PR.owned(f, R)).sum() > 20  # gaps between the rays
    touches, not_monotone = 0, 0
    for r in range(R):
        se, n_e = PR.rows_of(e, r)
        sf, n_f = PR.rows_of(f, r)
        t, w = e["t"][se:se + n_e].astype(np.float64), e["width"][se:se + n_e]
        assert ((t * 64 - 0.5) % 1 == 0).all() and (w == f32(1 / 64)).all() and (np.diff(t) > 0).all()
        assert n_e < 63 or (np.diff(t) > 1 / 64).any()  # holes
        tf = f["t"][sf:sf + n_f].astype(np.float64)
        assert (np.diff(tf) >= 0).all() and np.isin(f["width"][sf:sf + n_f], f32([0, 1 / 512, 1 / 256, 1 / 128])).all()
        if length[r] > 0 and n_e and n_f:
            lo_e, hi_e = PR.intervals(e, r, length[r])
            lo, hi = PR.intervals(f, r, length[r])
            touches += int(np.isin(hi, lo_e).sum() + np.isin(lo, hi_e).sum())
            not_monotone += int((np.diff(lo) < 0).any())
        for lst, s, n in ((e, se, n_e), (f, sf, n_f)):
            ww = lst["w"][s:s + n]
            assert n < 63 or (np.isnan(ww).sum() >= 1 and (ww < 0).sum() >= 1 and (ww == 0).sum() >= 1)
    assert touches > 1000 and not_monotone > 300, (touches, not_monotone)


@pytest.mark.parametrize("R", [65, 1025])
def test_span_is_the_brute_force_overlap_set(R):
    """the envelopes of the test lists are monotone in lo and hi: [j0, j1) of the two binary searches is exactly the set of envelope rows j
    with lo_e_j < hi_i and lo_i < hi_e_j, found by testing all pairs; both indices lie in [0, n_e]; with |dir| = 0 every span is empty"""
    lib = PR.build_host()
    case = PR.make_case(R, seed=700 + R)
    got = PR.host_loss(lib, case)
    brute = PR.brute64(case, got)
    some = 0
    for r in range(R):
        se, n_e = PR.rows_of(case["e"], r)
        sf, n_f = PR.rows_of(case["f"], r)
        assert (np.diff(got["lo_e"][se:se + n_e]) >= 0).all() and (np.diff(got["hi_e"][se:se + n_e]) >= 0).all()
        span = got["span"][sf:sf + n_f]
        assert (span >= 0).all() and (span <= n_e).all()
        j = np.arange(n_e)[None, :]
        assert np.array_equal((span[:, :1] <= j) & (j < span[:, 1:]), brute["overlap"][r]), r
        some += int(brute["overlap"][r].sum())
    assert some > 1000
    r0 = R - 3  # |dir| = 0: intervals of no width
    sf, n_f = PR.rows_of(case["f"], r0)
    assert n_f == 65 and (got["span"][sf:sf + n_f, 1] <= got["span"][sf:sf + n_f, 0]).all()


def _covering_case(w_env):
    """one ray: 40 envelope rows that tile [1 / 64, 41 / 64] without a hole, 100 fine rows of positive width inside it (a fine row of NO
    width that sits exactly on the edge between two envelope rows overlaps neither by the SPAN rule: its span is empty)"""
    rng = np.random.default_rng(5)
    n_e, n_f = 40, 100
    e = {"P": n_e, "start": np.zeros(1, np.int32), "count": np.full(1, n_e, np.int32), "t": ((np.arange(1, n_e + 1) + 0.5) / 64).astype(f32),
         "deltas": np.full(n_e, 2.0 / 64, f32), "w": np.full(n_e, w_env, f32)}
    f = {"P": n_f, "start": np.zeros(1, np.int32), "count": np.full(1, n_f, np.int32), "t": (np.sort(rng.integers(16, 320, n_f)) / 512).astype(f32),
         "deltas": (rng.choice(f32([1 / 512, 1 / 256, 1 / 128]), n_f) * f32(2)).astype(f32), "w": rng.random(n_f).astype(f32)}
    return {"R": 1, "dir": f32([[0, 0, 2.0]]), "e": e, "f": f}


def test_twin_properties():
    """the loss is 0 and so is the adjoint when the envelope dominates (w_e = 1 on a list that covers the fine list); with an empty envelope the
    loss is sum v^2 / (v + eps); the adjoint is <= 0 everywhere for g_loss > 0 and 0 where w_e <= 0 or NaN; coef is <= 0"""
    lib = PR.build_host()
    g1 = np.ones(1, f32)
    got = PR.host_loss(lib, _covering_case(1.0), g_loss=g1)
    assert got["loss"][0] == 0 and (got["coef"] == 0).all() and (got["g_w_e"] == 0).all() and (got["span"][:, 1] > got["span"][:, 0]).all()
    weak = PR.host_loss(lib, _covering_case(0.01), g_loss=g1)
    assert weak["loss"][0] > 1 and (weak["g_w_e"] <= 0).all() and (weak["g_w_e"] < 0).sum() > 20
    for R in (65, 1025):
        case = PR.make_case(R, seed=700 + R)
        got = PR.host_loss(lib, case, g_loss=np.ones(R, f32))
        own = PR.owned(case["e"], R)
        with np.errstate(invalid="ignore"):
            dead = own & ~(case["e"]["w"] > 0)
        assert (got["g_w_e"][own] <= 0).all() and (got["g_w_e"][dead] == 0).all() and dead.sum() > 100 and (got["g_w_e"][own] < 0).sum() > 100
        assert (got["coef"][PR.owned(case["f"], R)] <= 0).all() and (got["loss"] >= 0).all()
        zero = PR.host_loss(lib, case, eps=0.0)  # a fine row without weight costs nothing, whatever ulp the envelope's prefix dips by (BOUND)
        weightless = PR.owned(case["f"], R) & (PR.positive(case["f"]["w"]) == 0)
        assert weightless.sum() > 1000 and (zero["coef"][weightless] == 0).all() and (got["coef"][weightless] == 0).all() and np.isfinite(zero["loss"]).all()
        empties = 0
        for r in range(R):
            (_, n_e), (sf, n_f) = PR.rows_of(case["e"], r), PR.rows_of(case["f"], r)
            if n_e == 0 and n_f > 0:
                v = PR.positive(case["f"]["w"][sf:sf + n_f]).astype(np.float64)
                want = (v * v / np.where(v > 0, v + np.float64(f32(PR.EPS)), 1.0)).sum()
                assert abs(float(got["loss"][r]) - want) <= 1e-5 * max(want, 1e-30), r
                empties += 1
        assert empties >= 7


def test_loss_and_adjoint_against_the_float64_brute_force():
    """loss (R,) and g_w_e (Pe,) of the twin against the float64 all-pairs reference at the project's fp32 bar of 1e-4, the metric
    max |x - ref| / max |ref| per array.  Measured maxima of the twin: loss 4.9e-7, g_w_e 2.7e-6."""
    lib = PR.build_host()
    worst = {"loss": 0.0, "g_w_e": 0.0}
    for R in (65, 1025):
        case = PR.make_case(R, seed=700 + R)
        for eps in (PR.EPS, 1e-3):
            got = PR.host_loss(lib, case, eps)
            brute = PR.brute64(case, got, eps)
            own = PR.owned(case["e"], R)
            for k, x, ref in (("loss", got["loss"], brute["loss"]), ("g_w_e", got["g_w_e"][own], brute["g_w_e"][own])):
                err = PR.rel_err(x, ref)
                worst[k] = max(worst[k], err)
                assert np.abs(ref).max() > 1 and err <= PR.BAR, (R, eps, k, err)
    print("proposal loss against float64:", {k: "%.2e" % v for k, v in worst.items()})


def test_weights_backward_twin_against_float64_autograd():
    """proposal_host_weights_backward (the host's expf) against float64 autograd through the oracle's compute_weights on the same rays, at
    the same bar and metric, with and without g_trans; a NaN, a negative and a zero density get no gradient; the rows of no ray keep
    their sentinel; a NaN in g_w propagates to the rows of its ray and to no other.  Measured maximum of the twin: 8.3e-8."""
    lib = PR.build_host()
    lst, density, g_w, g_trans = PR.weights_case()
    R = lst["start"].shape[0]
    own = PR.owned(lst, R)
    worst = 0.0
    for gt in (None, g_trans):
        got = PR.host_weights_backward(lib, density, lst["deltas"], lst["start"], lst["count"], lst["P"], g_w, gt)
        ref = PR.weights_backward64(lst, density, g_w, gt)
        err = PR.rel_err(got[own], ref[own])
        worst = max(worst, err)
        assert (got[~own] == PR.SENTINEL_F).all() and np.abs(ref).max() > 1e-2 and err <= PR.BAR, err
        s3, _ = PR.rows_of(lst, 3)
        assert got[s3 + 1] == 0 and got[s3 + 2] == 0 and got[s3 + 5] == 0 and (got[own] != 0).sum() > 1000
    print("weights adjoint against float64 autograd: %.2e" % worst)
    bad = g_w.copy()
    s4, n4 = PR.rows_of(lst, 4)
    bad[s4 + n4 - 1] = np.nan
    got = PR.host_weights_backward(lib, density, lst["deltas"], lst["start"], lst["count"], lst["P"], bad, g_trans)
    with np.errstate(invalid="ignore"):
        counted = density[s4:s4 + n4] * lst["deltas"][s4:s4 + n4] > 0
    rest = own.copy()
    rest[s4:s4 + n4] = False
    assert n4 >= 63 and np.isnan(got[s4:s4 + n4][counted]).all() and not np.isnan(got[rest]).any()


def test_sanitized_standalone_program():
    """tests/host_harness/proposal_host_main.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, as a child process with its own main:
    NaN / negative / infinite weights, non-monotone envelopes with NaN and infinite t, a (start, count) outside [0, P), |dir| = 0;
    exact-size heap buffers"""
    r = subprocess.run([host_twin.sanitized_main("proposal")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "proposal_host_main: ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])


NAMES = ("weights_backward", "envelope", "proposal_forward", "proposal_backward")


def test_call_sites_and_prototypes_of_the_four_entry_points():
    """the entry points are declared with a stream, their signatures are the pinned ones, lab4d_amd/packed.py calls each with as many
    arguments as the prototype has in front of its stream, and the twin's definitions take the same parameters, stream aside"""
    import ast
    import ctypes
    from lab4d_amd import _lib
    vp, cl, ci, cf = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_float
    pinned = {"lab4d_packed_weights_backward": (ci, [vp] * 4 + [cl, cl] + [vp] * 4, True),
              "lab4d_packed_envelope": (ci, [vp] * 6 + [cl, cl] + [vp] * 4, True),
              "lab4d_packed_proposal_forward": (ci, [vp] * 5 + [cl] + [vp] * 5 + [cl, vp, cl, cf] + [vp] * 4, True),
              "lab4d_packed_proposal_backward": (ci, [vp] * 6 + [cl, vp, vp, cl, cl, vp, vp], True)}
    for name, want in pinned.items():
        restype, params, has_stream = _lib.SIGNATURES[name]
        assert (restype, _lib.argtypes(params), has_stream) == want, name
    sites = {}
    for node in ast.walk(ast.parse(open(os.path.join(_lib.HERE, "packed.py")).read())):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "call" and isinstance(node.func.value, ast.Name)
                and node.func.value.id == "_lib" and isinstance(node.args[0], ast.Constant) and node.args[0].value in ["packed_" + n for n in NAMES]):
            assert not any(isinstance(a, ast.Starred) for a in node.args)
            sites.setdefault(node.args[0].value, []).append(len(node.args) - 1)
    assert sites == {"packed_weights_backward": [9], "packed_envelope": [11], "packed_proposal_forward": [18], "packed_proposal_backward": [12]}, sites
    with open(os.path.join(host_twin.HARNESS, PR.TWIN + "_host.cpp")) as fh:
        text = fh.read()
    twin = host_twin.signatures(text, PR.TWIN + "_host.cpp")
    mine = {"weights_backward": "weights_backward", "envelope": "envelope", "proposal_forward": "forward", "proposal_backward": "backward"}
    assert sorted(twin) == sorted("proposal_host_" + v for v in mine.values()) and text.count('extern "C"') == 4
    lib = PR.build_host()
    for theirs, short in mine.items():
        assert twin["proposal_host_" + short][1] == _lib.argtypes(_lib.SIGNATURES["lab4d_packed_" + theirs][1])[:-1], short
        assert list(getattr(lib, "proposal_host_" + short).argtypes) == twin["proposal_host_" + short][1] and getattr(lib, "proposal_host_" + short).restype is None
    header = open(os.path.join(_lib.INCLUDE, "lab4d_hip.h")).read()
    assert '#include "lab4d_proposal.h"' in header and "struct" not in open(os.path.join(_lib.INCLUDE, "lab4d_proposal.h")).read().split("#ifndef")[1]


def test_library_checks_its_arguments_before_any_launch():
    """argument validation happens before any launch, so it runs without a GPU (tests/test_abi.py builds the library the same way)"""
    import ctypes
    from lab4d_amd import _lib
    _lib.build(verbose=False)
    so = ctypes.CDLL(_lib.SO_PATH)
    so.lab4d_last_error.restype = ctypes.c_char_p
    for name in NAMES:
        fn = getattr(so, "lab4d_packed_" + name)
        fn.restype, fn.argtypes = ctypes.c_int, _lib.argtypes(_lib.SIGNATURES["lab4d_packed_" + name][1])
    buf = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    err = so.lab4d_last_error

    def wb(R=1, P=4, rs=buf, g=buf):
        return so.lab4d_packed_weights_backward(buf, buf, rs, buf, R, P, buf, None, g, None)

    def env(R=1, Pe=4, d=buf, lo=buf):
        return so.lab4d_packed_envelope(buf, buf, buf, buf, buf, d, R, Pe, lo, buf, buf, None)

    def fwd(R=1, Pe=4, Pf=4, eps=1e-7, loss=buf, span=buf, lo=buf):
        return so.lab4d_packed_proposal_forward(lo, buf, buf, buf, buf, Pe, buf, buf, buf, buf, buf, Pf, buf, R, eps, span, buf, loss, None)

    def bwd(R=1, Pe=4, Pf=4, g=buf, out=buf, coef=buf):
        return so.lab4d_packed_proposal_backward(g, buf, coef, buf, buf, buf, Pe, buf, buf, Pf, R, out, None)

    for R, P, word in ((-1, 4, b"R = -1"), (1 << 31, 4, b"R = "), (1, -1, b" = -1"), (1, 1 << 31, b" = 2147483648")):
        for fn in (lambda: wb(R, P), lambda: env(R, P), lambda: fwd(R, P), lambda: fwd(R, 4, P), lambda: bwd(R, P), lambda: bwd(R, 4, P)):
            assert fn() == -1 and word in err(), (word, err())
    for eps in (-1e-5, float("nan"), float("inf")):
        assert fwd(eps=eps) == -1 and b"eps" in err()
    for fn in (lambda: wb(rs=None), lambda: wb(g=None), lambda: env(d=None), lambda: env(lo=None), lambda: fwd(loss=None), lambda: fwd(span=None), lambda: fwd(lo=None),
               lambda: bwd(g=None), lambda: bwd(out=None), lambda: bwd(coef=None)):
        assert fn() == -1 and b"null" in err(), err()
    # no rays: nothing to launch, nothing is required
    assert so.lab4d_packed_weights_backward(None, None, None, None, 0, 4, None, None, None, None) == 0
    assert so.lab4d_packed_envelope(None, None, None, None, None, None, 0, 4, None, None, None, None) == 0
    assert so.lab4d_packed_proposal_forward(None, None, None, None, None, 4, None, None, None, None, None, 4, None, 0, 0.0, None, None, None, None) == 0
    assert so.lab4d_packed_proposal_backward(None, None, None, None, None, None, 4, None, None, 4, 0, None, None) == 0


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
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.proposal_loss(_List(), z(6), _List(P=8), z(8), z(2, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        packed.render_weights(z(6), z(6), _List())
    cases = ((dict(rays_env=_List(t=z(6, dtype=torch.float64))), r"rays_env\.t must be float32"), (dict(rays_fine=_List(P=8, deltas=z(8, 1))), r"rays_fine\.deltas must be float32"),
             (dict(rays_env=_List(deltas=z(5))), "disagree on the number of rows"), (dict(rays_fine=_List(P=8, ray_start=z(2, dtype=torch.int64))), "must be int32"),
             (dict(w_env=z(5)), "w_env must be float32"), (dict(w_fine=z(8, dtype=torch.float16)), "w_fine must be float32"), (dict(w_fine=z(6)), "w_fine must be float32"),
             (dict(rays_fine=_List(P=8, R=3)), "disagree on the number of rays"), (dict(dir=z(2, 2)), r"dir must be float32 \(n, 3\)"),
             (dict(dir=z(3, 3)), "disagrees with the lists' 2 rays"), (dict(dir=z(2, 3, dtype=torch.float64)), "dir must be float32"),
             (dict(eps=-1.0), "eps"), (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps"))
    for kw, word in cases:
        args = dict(rays_env=_List(), w_env=z(6), rays_fine=_List(P=8), w_fine=z(8), dir=z(2, 3))
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            packed.proposal_loss(**args)
    for kw, word in ((dict(density=z(6, dtype=torch.float16)), "density must be float32"), (dict(density=z(6, 1, 1)), "density must be float32"),
                     (dict(deltas=z(5)), "deltas must be float32"), (dict(rays=_List(ray_count=z(3, dtype=torch.int32))), "must be int32")):
        args = dict(density=z(6), deltas=z(6), rays=_List())
        args.update(kw)
        with pytest.raises(RuntimeError, match=word):
            packed.render_weights(**args)
    sig = inspect.signature(packed.proposal_loss)
    assert list(sig.parameters) == ["rays_env", "w_env", "rays_fine", "w_fine", "dir", "eps"] and sig.parameters["eps"].default == torch.finfo(torch.float32).eps
    assert list(inspect.signature(packed.render_weights).parameters) == ["density", "deltas", "rays", "with_trans"]
    sig = inspect.signature(hashfield.render_packed_proposal)
    assert list(sig.parameters)[:14] == ["Pp", "cfgp", "P", "cfg", "grid", "origin", "dir", "t_range", "dt", "cap", "n_imp", "fine_cap", "u", "eps"]
    assert sig.parameters["eps"].default == 1e-5 and sig.parameters["fine_cap"].default is None and sig.parameters["u"].default is None


def test_kernels_have_no_private_segment_and_no_spills(tmp_path):
    kernels = host_twin.kernel_metadata("proposal.hip", tmp_path)
    names = [k["name"] for k in kernels]
    want = ("k_packed_weights_bwd", "k_packed_envelope", "k_packed_proposal_fwd", "k_packed_proposal_bwd")
    assert len(names) == 4 and all(any(n in x for x in names) for n in want), names
    for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "agpr_count"):
        assert {k[key] for k in kernels} == {0}, (key, kernels)
    assert max(k["vgpr_count"] for k in kernels) <= 64, kernels  # eight waves per SIMD by the vector registers
