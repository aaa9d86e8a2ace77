"""FeatureNeRF.global_match (nnutils/feature.py:152-199) as kernels (csrc/match.hip) against the oracle in float64, at the shapes where
their dispatch changes: every instantiation of the candidate-side backward kernel and both sides of each edge of its owner stride and of
the forward LDS tile, ray counts that take its ray loop through several LDS tiles (with short and empty blocks), three temperatures, a
single candidate, and candidates that all point away from the pixel features (row maxima below -88.7, where the weight of a padded
candidate register overflows); and the row tap that feeds it the drawn candidates, on every branch of its backward.

For every output and gradient tensor: e_dev <= max(1e-4, 2 e_ref), e_ref being the float32 oracle's distance from the same float64 truth
(tests/match_cases.py; tests/test_match_cases_cpu.py holds e_ref <= 5e-5, so the bound is 1e-4) -- relative L2, but for g_logsigma the
error over the un-cancelled magnitude of the sum it is -- and, for out, g_feat_c and g_xyz_c, element-wise
|device - truth64| <= 1e-5 max|truth64| + 1e-4 |truth64|.  Where the truth is identically zero the device must be too: with one candidate
the kernel forms the softmax's adjoint as one difference that vanishes exactly (match.hip, k_match_bwd_cand).

Measured on the MI355X, worst e_dev over the 42 cases (parity_match_*.json): out 6.5e-6, stats 8.1e-8 (maximum) and 6.7e-6 (sum),
g_feat_c 5.0e-6, g_xyz_c 4.6e-6, g_logsigma 4.3e-7 of its un-cancelled magnitude; e_ref is at most 6.8e-6, so every bound is 1e-4."""
import pytest
import torch

import match_cases as MC
from parity_report import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = -7.0
GUARD = 3  # rows after the end of every output


def _raw_forward(inp, R, K, out, stats, C=MC.C):
    from lab4d_amd import _lib
    try:
        _lib.call("global_match_forward", inp["feat_px"], inp["feat_c"], inp["xyz_c"], inp["logsigma"], R, C, K, out, stats)
    finally:
        torch.cuda.synchronize()


def _raw_backward(inp, out, stats, R, K, g_fc, g_xc, g_ls, work, C=MC.C):
    from lab4d_amd import _lib
    try:
        _lib.call("global_match_backward", inp["feat_px"], inp["feat_c"], inp["xyz_c"], inp["logsigma"], out, stats, inp["w"], R, C, K,
                  g_fc, g_xc, g_ls, work)
    finally:
        torch.cuda.synchronize()


def _on_device(case):
    return {k: v.to(DEV) for k, v in MC.inputs(case).items()}


def _device_match(f, fc, xc, ls):
    from lab4d_amd import deformable as DF
    return DF.GlobalMatch.apply(f, fc, xc, ls)


def _device_results(case):
    """Every name of match_cases.TENSORS from the device: out and the gradients through GlobalMatch.apply, stats from the entry point."""
    dev = MC.run_match(_device_match, MC.inputs(case), torch.float32, DEV)
    inp = _on_device(case)
    out, stats = torch.full((case.R, 3), FILL, device=DEV), torch.full((case.R, 2), FILL, device=DEV)
    _raw_forward(inp, case.R, case.K, out, stats)
    assert torch.equal(out, dev["out"]), "the entry point and GlobalMatch.apply are the same launch"
    dev["stats_max"], dev["stats_sum"] = stats[:, 0], stats[:, 1]
    return dev


def held(case, dev=None):
    """Report e_dev, e_ref and their ratio per tensor, then assert the bounds of the module docstring.  -> name -> e_dev."""
    truth, ref32, A = MC.reference(case)
    dev = _device_results(case) if dev is None else dev
    assert set(dev) == set(truth)
    measured, bad = {}, {}
    for k in MC.TENSORS:
        d, t = dev[k].detach().double().cpu(), truth[k]
        assert d.shape == t.shape, (k, d.shape, t.shape)
        e_dev, e_ref = MC.error(k, d, truth, A), MC.error(k, ref32[k], truth, A)
        measured[k + ".e_dev"], measured[k + ".e_ref"], measured[k + ".ratio"] = e_dev, e_ref, (e_dev / e_ref if e_ref > 0 else 0.0)
        tmax = float(t.abs().max())
        excess = float(((d - t).abs() - (1e-5 * tmax + 1e-4 * t.abs())).max()) if k in MC.ELEMENTWISE else 0.0
        measured[k + ".maxabs_over_max"] = float((d - t).abs().max()) / tmax if tmax > 0 else float(d.abs().max())
        zero_ok = tmax > 0 or float(d.abs().max()) == 0
        if not (e_dev <= MC.bound(e_ref) and excess <= 0 and zero_ok):
            bad[k] = (e_dev, e_ref, excess, zero_ok)
    report("match_" + case.name, measured)
    assert not bad, "%s: (e_dev, e_ref, element-wise excess, zero where the truth is zero) %s" % (case.name, bad)
    assert bool((dev["stats_sum"] >= 1).all()), "the row maximum contributes exp(0) to the sum of exponentials"
    return measured


@pytest.mark.parametrize("case", [c for c in MC.CASES if c not in MC.FIRST or c in MC.CONSTANT], ids=lambda c: c.name)
def test_global_match_float64_parity(case):
    dev = _device_results(case)
    held(case, dev)
    if case.K == 1:  # the softmax is constant: nothing reaches the features or the temperature, and out is the candidate's point
        assert torch.equal(dev["out"].cpu(), MC.inputs(case)["xyz_c"].expand(case.R, 3))
        assert float(dev["g_feat_c"].abs().max()) == 0 and float(dev["g_logsigma"].abs().max()) == 0
        assert bool((dev["stats_sum"] == 1).all())


@pytest.mark.parametrize("R,K", MC.FIRST_SHAPES)
def test_global_match_equals_the_reference_expression(R, K):
    """The shapes and the two temperatures this kernel was first tested at, under the rule of the module docstring; and, as then, the
    largest deviation of out within 1e-5 and of the gradient tensors within 2e-5 of the largest entry -- now of the float64 truth, and with
    no floor under that entry: where it is zero (one candidate) the device is exactly zero."""
    for case in [c for c in MC.FIRST if (c.R, c.K) == (R, K)]:
        m = held(case)
        assert m["out.maxabs_over_max"] < 1e-5, (case.name, m["out.maxabs_over_max"])
        for k in ("g_feat_c", "g_xyz_c"):
            assert m[k + ".maxabs_over_max"] < 2e-5, (case.name, k, m[k + ".maxabs_over_max"])
        # the scalar as then, too: within 2e-5 of its own value or of 5e-2 (at these shapes it does not cancel below that by much)
        t = abs(float(MC.reference(case)[0]["g_logsigma"]))
        assert m["g_logsigma.maxabs_over_max"] * (t if t > 0 else 1.0) < 2e-5 * max(t, 5e-2), (case.name, m["g_logsigma.maxabs_over_max"], t)


def test_global_match_is_deterministic():
    from lab4d_amd import deformable as DF
    feat_px = torch.randn(3000, 16, device=DEV)
    fc, xc = torch.randn(1024, 16, device=DEV, requires_grad=True), torch.randn(1024, 3, device=DEV, requires_grad=True)
    ls = torch.zeros(1, device=DEV, requires_grad=True)
    res = []
    for _ in range(2):
        out = DF.GlobalMatch.apply(feat_px, fc, xc, ls)
        res.append([out.detach()] + [t.clone() for t in torch.autograd.grad(out.square().sum(), [fc, xc, ls])])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_global_match_is_deterministic_across_ray_tiles():
    """R = 16449, K = 700: every block sums over two LDS tiles, the reduction over 256 partials of which two are zero."""
    case = MC.DETERMINISM_CASE
    res = [MC.run_match(_device_match, MC.inputs(case), torch.float32, DEV) for _ in range(2)]
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k


# ---------------------------------------------------------------------------------------------------
# the entry points themselves: what they write, and what they refuse
# ---------------------------------------------------------------------------------------------------


def _filled(*shape):
    return torch.full(shape, FILL, device=DEV)


@pytest.mark.parametrize("case", MC.WRITTEN_CASES, ids=lambda c: c.name)
def test_every_output_element_is_written_and_nothing_beyond(case):
    from lab4d_amd import _lib
    R, K = case.R, case.K
    inp = _on_device(case)
    truth, _, A = MC.reference(case)
    out, stats = _filled(R + GUARD, 3), _filled(R + GUARD, 2)
    _raw_forward(inp, R, K, out, stats)
    W = _lib.lib().lab4d_global_match_workspace_floats(K)
    assert W == 256 * K * 20
    g_fc, g_xc, g_ls, work = _filled(K + GUARD, MC.C), _filled(K + GUARD, 3), _filled(1 + GUARD), _filled(W + GUARD)
    _raw_backward(inp, out, stats, R, K, g_fc, g_xc, g_ls, work)
    for name, t, n in (("out", out, R), ("stats", stats, R), ("g_feat_c", g_fc, K), ("g_xyz_c", g_xc, K), ("g_logsigma", g_ls, 1), ("work", work, W)):
        assert bool((t[n:] == FILL).all()), "%s: written beyond its %d rows" % (name, n)
        if name != "work":
            assert bool((t[:n] != FILL).all()), "%s: not written everywhere" % name
    nb = MC.dispatch(R, K)["NB"]
    assert bool((work[:nb * K * 20] != FILL).all()), "every launched block writes its partials, the empty ones zeros"
    assert bool((work[nb * K * 20:] == FILL).all())
    # and what was written is the result
    dev = {"out": out[:R], "stats_max": stats[:R, 0], "stats_sum": stats[:R, 1], "g_feat_c": g_fc[:K], "g_xyz_c": g_xc[:K], "g_logsigma": g_ls[:1]}
    for k in MC.TENSORS:
        e = MC.error(k, dev[k], truth, A)
        assert e <= MC.NORTH_STAR_TOL, (k, e)


def test_no_rays():
    """R = 0: forward writes nothing; backward launches no candidate kernel and the reduction writes zeros."""
    from lab4d_amd import _lib
    K = 300
    inp = _on_device(MC.R_SWEEP[0])
    out, stats = _filled(GUARD, 3), _filled(GUARD, 2)
    _raw_forward(inp, 0, K, out, stats)
    assert bool((out == FILL).all()) and bool((stats == FILL).all())
    W = _lib.lib().lab4d_global_match_workspace_floats(K)
    g_fc, g_xc, g_ls, work = _filled(K + GUARD, MC.C), _filled(K + GUARD, 3), _filled(1 + GUARD), _filled(W + GUARD)
    _raw_backward(inp, out, stats, 0, K, g_fc, g_xc, g_ls, work)
    for t, n in ((g_fc, K), (g_xc, K), (g_ls, 1)):
        assert bool((t[:n] == 0).all()) and bool((t[n:] == FILL).all())
    assert bool((work == FILL).all())


def _misaligned(t):
    """The same values one float further on: a contiguous view whose address is 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 4, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def test_refusals_are_decided_before_any_launch():
    from lab4d_amd import _lib
    R, K = 5, 7
    inp = _on_device(MC._case(R, K))
    fwd_in = ("feat_px", "feat_c", "xyz_c", "logsigma")
    try:
        def forward(C=MC.C, K=K, **swap):
            a = dict(inp, out=_filled(R, 3), stats=_filled(R, 2))
            a.update(swap)
            with pytest.raises(RuntimeError, match="global_match_forward"):
                _lib.call("global_match_forward", *[a[k] for k in fwd_in], R, C, K, a["out"], a["stats"])
            torch.cuda.synchronize()
            assert all(bool((a[k] == FILL).all()) for k in ("out", "stats") if a[k] is not None)

        def backward(C=MC.C, K=K, **swap):
            a = dict(inp, out=torch.zeros(R, 3, device=DEV), stats=torch.ones(R, 2, device=DEV), g_fc=_filled(8, MC.C), g_xc=_filled(8, 3),
                     g_ls=_filled(1), work=_filled(_lib.lib().lab4d_global_match_workspace_floats(8)))
            a.update(swap)
            with pytest.raises(RuntimeError, match="global_match_backward"):
                _lib.call("global_match_backward", *[a[k] for k in fwd_in], a["out"], a["stats"], a["w"], R, C, K,
                          a["g_fc"], a["g_xc"], a["g_ls"], a["work"])
            torch.cuda.synchronize()
            assert all(bool((a[k] == FILL).all()) for k in ("g_fc", "g_xc", "g_ls", "work") if a[k] is not None)

        for fn in (forward, backward):
            fn(C=8)
            fn(K=0)
            fn(K=1025)
            fn(feat_px=_misaligned(inp["feat_px"]))
            fn(feat_c=_misaligned(inp["feat_c"]))
        for k in fwd_in + ("out", "stats"):
            forward(**{k: None})
        for k in fwd_in + ("out", "stats", "w", "g_fc", "g_xc", "g_ls", "work"):
            backward(**{k: None})
    finally:
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------
# RowTap
# ---------------------------------------------------------------------------------------------------
S = 5000


def _tap_setup(n_idx, duplicates=False, seed=11):
    g = MC.gen(seed)
    x = torch.randn(S, MC.C, generator=g).to(DEV).requires_grad_(True)
    idx = torch.randint(0, 50, (n_idx,), generator=g) if duplicates else torch.randperm(S, generator=g)[:n_idx]
    w, v = torch.randn(S, MC.C, generator=g), torch.randn(n_idx, MC.C, generator=g)
    return x, idx, w, v


def _tap_close(gx, dense, idx, v):
    """gx against dense.index_add(0, idx, v) in float64.  A row drawn n times is a sum of n + 1 float32 terms in some order: each addition
    rounds by at most 2^-24 of a partial sum, which the sum of the terms' magnitudes bounds."""
    truth = dense.double().index_add(0, idx, v.double())
    mag = dense.double().abs().index_add(0, idx, v.double().abs())
    n = int(torch.bincount(idx, minlength=S).max())
    err = (gx.detach().double().cpu() - truth).abs()
    assert bool((err <= n * 2.0 ** -24 * mag).all()), float((err - n * 2.0 ** -24 * mag).max())
    drawn = torch.zeros(S, dtype=torch.bool).index_fill_(0, idx, True)
    assert torch.equal(gx.detach().cpu()[~drawn], dense[~drawn]), "a row that was not drawn keeps the dense gradient bit for bit"


def test_row_tap_adds_the_rows_gradient_into_the_dense_one():
    from lab4d_amd import deformable as DF
    x = torch.randn(5000, 16, device=DEV, requires_grad=True)
    idx = torch.randperm(5000, device=DEV)[:1024]
    w, v = torch.randn(5000, 16, device=DEV), torch.randn(1024, 16, device=DEV)
    y, rows = DF.RowTap.apply(x, idx)
    assert torch.equal(y, x) and torch.equal(rows, x[idx])
    (gx,) = torch.autograd.grad((y * w).sum() + (y * 2).sum() + (rows * v).sum(), [x])
    ref = (w + 2).index_add(0, idx, v)
    assert torch.allclose(gx, ref, rtol=0, atol=1e-6)
    # only the rows are consumed: the dense gradient is built here
    y, rows = DF.RowTap.apply(x, idx)
    (gx,) = torch.autograd.grad((rows * v).sum(), [x])
    assert torch.allclose(gx, torch.zeros_like(x).index_add(0, idx, v))


@pytest.mark.parametrize("n_idx,duplicates", [(1, False), (1024, False), (1024, True)], ids=["one_row", "1024_rows", "1024_rows_of_50"])
def test_row_tap_float64_parity(n_idx, duplicates):
    """The dense gradient arrives from one consumer (autograd's own buffer: the in-place branch), and not at all."""
    from lab4d_amd import deformable as DF
    x, idx, w, v = _tap_setup(n_idx, duplicates)
    if duplicates:
        assert int(torch.bincount(idx).max()) > 20
    y, rows = DF.RowTap.apply(x, idx.to(DEV))
    assert torch.equal(y, x) and torch.equal(rows, x[idx.to(DEV)])
    (gx,) = torch.autograd.grad((y * w.to(DEV)).sum() + (rows * v.to(DEV)).sum(), [x])
    _tap_close(gx, w, idx, v)
    y, rows = DF.RowTap.apply(x, idx.to(DEV))
    (gx,) = torch.autograd.grad((rows * v.to(DEV)).sum(), [x])  # (c) g_dense is None
    _tap_close(gx, torch.zeros(S, MC.C), idx, v)


def test_row_tap_leaves_a_shared_gradient_buffer_alone():
    """(a) y + y2: AddBackward hands ONE tensor to both of its edges; the rows must not show up in the other consumer's gradient."""
    from lab4d_amd import deformable as DF
    for duplicates in (False, True):
        x, idx, w, v = _tap_setup(1024, duplicates, seed=12)
        y2 = torch.randn(S, MC.C, device=DEV, requires_grad=True)
        for order in (0, 1):
            y, rows = DF.RowTap.apply(x, idx.to(DEV))
            z = y + y2 if order == 0 else y2 + y
            gx, g2 = torch.autograd.grad((z * w.to(DEV)).sum() + (rows * v.to(DEV)).sum(), [x, y2])
            assert torch.equal(g2.cpu(), w), "the other consumer's gradient was changed by the in-place add"
            _tap_close(gx, w, idx, v)


def test_row_tap_copies_a_view_or_a_strided_gradient():
    """(b) the dense gradient arrives as a view of another tensor, or not contiguous."""
    from lab4d_amd import deformable as DF
    x, idx, w, v = _tap_setup(1024, True, seed=13)
    wd, vd = w.to(DEV), v.to(DEV)
    # through y.t().t(): the gradient is a view (of autograd's buffer) with contiguous strides
    y, rows = DF.RowTap.apply(x, idx.to(DEV))
    (gx,) = torch.autograd.grad((y.t().t() * wd).sum() + (rows * vd).sum(), [x])
    _tap_close(gx, w, idx, v)
    # an expanded cotangent: stride 0 along the rows
    row = torch.randn(1, MC.C, generator=MC.gen(14))
    cot = row.to(DEV).expand(S, MC.C)
    assert not cot.is_contiguous()
    y, rows = DF.RowTap.apply(x, idx.to(DEV))
    (gx,) = torch.autograd.grad([y, rows], [x], grad_outputs=[cot, vd])
    _tap_close(gx, row.expand(S, MC.C).contiguous(), idx, v)
    assert torch.equal(cot[0].cpu(), row[0]) and torch.equal(cot[S - 1].cpu(), row[0])
    # a transposed cotangent
    cot = wd.t().contiguous().t()
    assert not cot.is_contiguous()
    y, rows = DF.RowTap.apply(x, idx.to(DEV))
    (gx,) = torch.autograd.grad([y, rows], [x], grad_outputs=[cot, vd])
    _tap_close(gx, w, idx, v)
    assert torch.equal(cot.cpu(), w)
    # a contiguous slice of a larger buffer
    big = torch.cat([wd, wd], 0)
    y, rows = DF.RowTap.apply(x, idx.to(DEV))
    (gx,) = torch.autograd.grad([y, rows], [x], grad_outputs=[big[:S], vd])
    _tap_close(gx, w, idx, v)
    assert torch.equal(big.cpu(), torch.cat([w, w], 0))


def test_row_tap_leaves_the_callers_gradient_alone():
    """(d) grad_outputs belong to the caller: bit-identical after the call, through autograd.grad and through backward()."""
    from lab4d_amd import deformable as DF
    x, idx, w, v = _tap_setup(1024, True, seed=15)
    cot, vd = w.to(DEV), v.to(DEV)
    y, rows = DF.RowTap.apply(x, idx.to(DEV))
    (gx,) = torch.autograd.grad([y, rows], [x], grad_outputs=[cot, vd])
    assert torch.equal(cot.cpu(), w) and torch.equal(vd.cpu(), v)
    _tap_close(gx, w, idx, v)
    assert gx.data_ptr() != cot.data_ptr()
    y, rows = DF.RowTap.apply(x, idx.to(DEV))
    torch.autograd.backward([y, rows], [cot, vd])
    assert torch.equal(cot.cpu(), w) and torch.equal(vd.cpu(), v)
    _tap_close(x.grad, w, idx, v)
