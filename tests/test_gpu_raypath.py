"""Ray sampling and compositing kernels (csrc/raymarch.hip, csrc/composite.hip) against the oracle in float64, at the shapes where their
dispatch changes: every NC = ceil(D/64) of the compositing kernels and both sides of each chunk edge, the three channel classes of
field_reduce and its adjoint, degenerate rays, the grid-stride loops, NULL in every optional pointer slot, and the host-side refusals.

For every output and gradient tensor: e_dev = ||device - truth64|| / ||truth64|| <= max(1e-4, 2 e_ref), e_ref being the float32 oracle's
distance from the same truth (tests/raypath_cases.py; tests/test_raypath_cases_cpu.py holds e_ref <= 5e-5, so the bound is 1e-4), and
element-wise |device - truth64| <= 1e-5 max|truth64| + 1e-4 |truth64|.  Where the truth is identically zero the device must be too.  For the
three degenerate ray kinds the same two checks are repeated on the other rays alone: the gradients of an empty ray carry the factor
1 / (mask + 1e-6) = 1e6 and would otherwise set the scale of both."""
import pytest
import torch

import raypath_cases as RC
from oracle import lab4d_oracle as O
from parity_report import report
from test_gpu_ops import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = -7.0


def _errors(dev, truth, ref32, rows=None):
    """name -> (e_dev, e_ref, worst element-wise excess over atol + rtol |truth|, exact-zero verdict) for every tensor of the truth."""
    assert set(dev) == set(truth), (sorted(dev), sorted(truth))
    res = {}
    for k, t in truth.items():
        d, r = dev[k].detach().double().cpu(), ref32[k]
        assert d.shape == t.shape, (k, d.shape, t.shape)
        if rows is not None:
            d, t, r = (x.reshape(len(rows), -1)[rows] for x in (d, t, r))
        tmax = float(t.abs().max()) if t.numel() else 0.0
        excess = float(((d - t).abs() - (1e-5 * tmax + 1e-4 * t.abs())).max()) if t.numel() else 0.0
        res[k] = (RC.rel_l2(d, t), RC.rel_l2(r, t), excess, tmax > 0 or float(d.abs().max()) == 0)
    return res


def held(tag, dev, truth, ref32, rows=None):
    """Report e_dev, e_ref and their ratio per tensor, then assert the bounds of the module docstring."""
    res = _errors(dev, truth, ref32, rows)
    measured = {}
    for k, (e_dev, e_ref, _, _) in res.items():
        measured[k + ".e_dev"], measured[k + ".e_ref"] = e_dev, e_ref
        measured[k + ".ratio"] = e_dev / e_ref if e_ref > 0 else 0.0
    report("raypath_" + tag, measured)
    bad = {k: v for k, v in res.items() if not (v[0] <= RC.bound(v[1]) and v[2] <= 0 and v[3])}
    assert not bad, "%s: (e_dev, e_ref, element-wise excess, zero where the truth is zero) %s" % (tag, bad)


# ---------------------------------------------------------------------------------------------------
# compositing
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", RC.COMPOSITE_CASES, ids=lambda c: c.name)
def test_render_pixel_float64_parity(case):
    from lab4d_amd import render_utils as RU
    truth, ref32 = RC.composite_reference(case)
    out, grads = RC.run_render_pixel(RU.render_pixel, RC.composite_inputs(case), torch.float32, DEV)
    dev = RC._tensors(out, grads)
    held(case.name, dev, truth, ref32)
    if case.kind != "plain":
        R = case.M * case.N
        bad = RC.BAD_RAY[0] * case.N + RC.BAD_RAY[1]
        held(case.name + "_other_rays", dev, truth, ref32, rows=torch.arange(R) != bad)


@pytest.mark.parametrize("D", RC.WEIGHTS_D)
def test_compute_weights_float64_parity(D):
    """_Weights: device forward, Python adjoint."""
    from lab4d_amd import render_utils as RU
    truth, ref32 = RC.weights_reference(D)
    dev = RC.run_compute_weights(RU.compute_weights, RC.weights_inputs(D), torch.float32, DEV)
    held("weights_d%d" % D, dev, truth, ref32)
    err = float((dev["out.weights"].sum(-1) + dev["out.transmit"][..., -1] - 1).abs().max())
    assert err < 1e-5, err


def test_composite_grid_stride_rays_beyond_the_first_pass():
    """R = 65541 > 16384 blocks x 4 rays: the rays of the second pass of the grid-stride loop, forward and backward."""
    from lab4d_amd import render_utils as RU
    M, N, D = RC.GRID_STRIDE_COMPOSITE
    g = RC.gen(5)
    inputs = {"density": torch.rand(M, N, D, 1, generator=g) * 600.0 / D, "rgb": torch.rand(M, N, D, 3, generator=g),
              "vis": torch.randn(M, N, D, 1, generator=g) * 3, "deltas": torch.rand(M, N, D, 1, generator=g) * 0.02}
    ref = RC._tensors(*RC.run_render_pixel(O.render_pixel, inputs))
    dev = RC._tensors(*RC.run_render_pixel(RU.render_pixel, inputs, torch.float32, DEV))
    assert set(dev) == set(ref)
    first = 16384 * 4
    for k, r in ref.items():
        close(dev[k], r, k)
        close(dev[k].reshape(N, -1)[first:], r.reshape(N, -1)[first:], k + " beyond the first %d rays" % first)


def _raw_composite(case):
    """Device tensors and the field list of one case, as _Composite hands them to the C ABI."""
    from lab4d_amd import _lib
    inp = {k: v.to(DEV) for k, v in RC.composite_inputs(case).items()}
    fd = RC.field_dict_of(inp)
    plan = RC.composited_fields(case)
    fields = [fd[k].contiguous() for k, _, _ in plan]
    fl = _lib.FieldList()
    fl.n_fields = len(plan)
    for i, ((k, C, mode), f) in enumerate(zip(plan, fields)):
        fl.fields[i], fl.channels[i], fl.modes[i] = f.data_ptr(), C, mode
    sumC = sum(1 if m == 2 else C for _, C, m in plan)
    a = {"density": fd["density"], "deltas": inp["deltas"], "flow": fd["flow"].contiguous(), "vis": fd["vis"], "gdens": fd["gauss_density"]}
    return a, plan, fields, fl, sumC


def _composite_backward(case, cot, without=()):
    """One launch of composite_backward into outputs pre-filled with FILL; `without` names the gradient outputs handed over as NULL."""
    from lab4d_amd import _lib
    a, plan, fields, fl, sumC = _raw_composite(case)
    outs = {"g_density": a["density"], "g_deltas": a["deltas"], "g_flow": a["flow"], "g_vis": a["vis"], "g_gdens": a["gdens"]}
    outs.update({"field." + k: f for (k, _, _), f in zip(plan, fields)})
    outs = {k: (None if k in without else torch.full_like(v, FILL)) for k, v in outs.items()}
    gf = _lib.FieldGrads()
    gf.n_fields = len(plan)
    for i, (k, _, _) in enumerate(plan):
        g = outs["field." + k]
        gf.fields[i] = g.data_ptr() if g is not None else None
    _lib.call("composite_backward", a["density"], a["deltas"], fl, a["flow"], a["vis"], a["gdens"], case.M * case.N, case.D,
              cot["g_mask"], cot["g_out"], cot["g_flow_out"], cot["g_vis_num"], cot["g_gauss_mask"],
              outs["g_density"], outs["g_deltas"], gf, outs["g_flow"], outs["g_vis"], outs["g_gdens"])
    torch.cuda.synchronize()
    return {k: v for k, v in outs.items() if v is not None}


def _composite_cotangents(case):
    _, _, _, _, sumC = _raw_composite(case)
    g = RC.gen(6)
    R = case.M * case.N
    return {k: torch.randn(R, c, generator=g).to(DEV) for k, c in [("g_mask", 1), ("g_out", sumC), ("g_flow_out", 2), ("g_vis_num", 1), ("g_gauss_mask", 1)]}


def _same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)
        assert bool((a[k] != FILL).all()), "%s: %s was not written everywhere" % (what, k)


def test_composite_backward_null_cotangent_equals_zero_cotangent():
    case = RC.NULL_CASE
    cot = _composite_cotangents(case)
    for names in [(k,) for k in cot] + [tuple(cot)]:
        zero = {k: (torch.zeros_like(v) if k in names else v) for k, v in cot.items()}
        null = {k: (None if k in names else v) for k, v in cot.items()}
        _same(_composite_backward(case, zero), _composite_backward(case, null), "NULL %s" % (names,))


def test_composite_backward_null_gradient_output_leaves_the_others_alone():
    case = RC.NULL_CASE
    cot = _composite_cotangents(case)
    full = _composite_backward(case, cot)
    optional = [k for k in full if k.startswith("field.")] + ["g_flow", "g_vis", "g_gdens"]
    assert len(optional) == len(RC.composited_fields(case)) + 3
    for k in optional:
        part = _composite_backward(case, cot, without=(k,))
        assert k not in part
        _same(part, {n: v for n, v in full.items() if n != k}, "without " + k)


def _composite_forward(case, D=None, without=()):
    from lab4d_amd import _lib
    a, plan, fields, fl, sumC = _raw_composite(case)
    M, N, dev = case.M, case.N, DEV
    shapes = {"weights": (M, N, case.D), "transmit": (M, N, case.D), "mask": (M, N, 1), "out": (M, N, sumC), "flow_out": (M, N, 2),
              "vis_num": (M, N, 1), "t_sum": (M, N, 1), "gauss_mask": (M, N, 1)}
    outs = {k: (None if k in without else torch.full(s, FILL, device=dev)) for k, s in shapes.items()}
    try:
        _lib.call("composite_forward", a["density"], a["deltas"], fl, a["flow"], a["vis"], a["gdens"], M * N, case.D if D is None else D,
                  *[outs[k] for k in shapes])
    finally:
        torch.cuda.synchronize()
    return {k: v for k, v in outs.items() if v is not None}


def test_composite_forward_null_outputs_leave_the_others_alone():
    case = RC.NULL_CASE
    full = _composite_forward(case)
    truth, _ = RC.composite_reference(case)
    close(full["mask"], truth["out.mask"].float(), "raw forward mask")
    for names in [("weights",), ("transmit",), ("mask",), ("weights", "transmit", "mask")]:
        part = _composite_forward(case, without=names)
        _same(part, {n: v for n, v in full.items() if n not in names}, "without %s" % (names,))


# ---------------------------------------------------------------------------------------------------
# ray sampling
# ---------------------------------------------------------------------------------------------------


def _dev_ray_samples(hxy, K, nf, c2f, D, depth):
    from lab4d_amd import render_utils as RU
    return RU.ray_samples(hxy, K, nf, c2f, n_depth=D, depth=depth)


def _dev_cam_rays(hxy, K, nf, D, depth):
    from lab4d_amd import render_utils as RU
    return RU.sample_cam_rays(hxy, K, nf, n_depth=D, depth=depth)


@pytest.mark.parametrize("case", RC.RAY_CASES, ids=lambda c: c.name)
def test_ray_samples_float64_parity(case):
    truth, ref32 = RC.ray_reference(case)
    inp = RC.ray_inputs(case)
    dev = RC.run_ray_samples(_dev_ray_samples, inp, case.D, torch.float32, DEV)
    # the sample positions first: the float64 truth was given the float32 oracle's depth, so the device has to reproduce that
    d, r = dev["out.depth"].cpu(), ref32["out.depth"]
    report("raypath_depth_" + case.name, {"not_bit_equal": float((d != r).sum()), "elements": float(r.numel())})
    torch.testing.assert_close(d, r, rtol=1e-6, atol=0)
    held("rays_" + case.name, dev, truth, ref32)
    truth_u, ref_u = RC.cam_rays_reference(case)
    held("camrays_" + case.name, RC.run_cam_rays(_dev_cam_rays, inp, case.D, torch.float32, DEV), truth_u, ref_u)


def test_ray_samples_grid_stride_samples_beyond_the_first_pass():
    """S = 2,099,200 > 8192 blocks x 256 samples: the samples of the second pass of the grid-stride loop (forward only)."""
    M, N, D = RC.GRID_STRIDE_RAYS
    inp = RC.ray_inputs(RC.RayCase("grid", M, N, D, False, True), with_cot=False)
    with torch.no_grad():
        ref = RC.oracle_ray_samples(inp["hxy"], inp["Kinv"], inp["near_far"], (inp["cq"], inp["ct"]), D)
        dev = _dev_ray_samples(inp["hxy"].to(DEV), inp["Kinv"].to(DEV), inp["near_far"].to(DEV), (inp["cq"].to(DEV), inp["ct"].to(DEV)), D, None)
    first = 8192 * 256
    assert M * N * D > first
    for d, r, k in zip(dev, ref, RC.RAY_OUTPUTS):
        close(d, r, k)
        close(d.reshape(M * N * D, -1)[first:], r.reshape(M * N * D, -1)[first:], k + " beyond the first %d samples" % first)


def _ray_backward(inp, D, cot, without=()):
    """One launch of ray_samples_backward onto zeroed accumulators, as _RaySamples.backward does."""
    from lab4d_amd import _lib
    M, N = inp["hxy"].shape[:2]
    outs = {"g_Kinv": (M, 3, 3), "g_q": (M, 4), "g_t": (M, 3)}
    outs = {k: (None if k in without else torch.zeros(s, device=DEV)) for k, s in outs.items()}
    _lib.call("ray_samples_backward", inp["hxy"], inp["Kinv"], inp["near_far"], None, inp["cq"], inp["ct"], M, N, D,
              cot["g_xyz_cam"], cot["g_dir_cam"], cot["g_deltas"], cot["g_xyz_field"], cot["g_dir_field"], outs["g_Kinv"], outs["g_q"], outs["g_t"])
    torch.cuda.synchronize()
    return {k: v for k, v in outs.items() if v is not None}


def _ray_null_setup():
    case = RC.NULL_RAY_CASE
    inp = RC.ray_inputs(case)
    cot = {k: c.float().to(DEV) for k, c in zip(("g_xyz_cam", "g_dir_cam", "g_deltas", "g_xyz_field", "g_dir_field"), inp["cot"])}
    return case, {k: v.to(DEV) for k, v in inp.items() if k in ("hxy", "Kinv", "near_far", "cq", "ct")}, cot


def _equal(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


def test_ray_samples_backward_null_cotangent_equals_zero_cotangent():
    """N = 65: two blocks per frame add onto a zeroed accumulator -- a sum of two terms is the same in either order."""
    case, inp, cot = _ray_null_setup()
    for names in [(k,) for k in cot] + [tuple(cot)]:
        zero = {k: (torch.zeros_like(v) if k in names else v) for k, v in cot.items()}
        null = {k: (None if k in names else v) for k, v in cot.items()}
        _equal(_ray_backward(inp, case.D, zero), _ray_backward(inp, case.D, null), "NULL %s" % (names,))


def test_ray_samples_backward_null_gradient_output_leaves_the_others_alone():
    case, inp, cot = _ray_null_setup()
    full = _ray_backward(inp, case.D, cot)
    assert all(float(v.abs().min()) > 0 for v in full.values()), "every accumulator entry receives something"
    for k in ("g_Kinv", "g_q", "g_t"):
        part = _ray_backward(inp, case.D, cot, without=(k,))
        assert k not in part
        _equal(part, {n: v for n, v in full.items() if n != k}, "without " + k)


# ---------------------------------------------------------------------------------------------------
# sort_depth
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name,a,b", RC.sort_depth_cases(), ids=[c[0] for c in RC.sort_depth_cases()])
def test_sort_depth_equals_torch_sort(name, a, b):
    from lab4d_amd import render_utils as RU
    out = RU.sort_depth(a.to(DEV), b.to(DEV)).cpu()
    assert torch.equal(out, torch.sort(torch.cat([a, b], -1), -1)[0])


# ---------------------------------------------------------------------------------------------------
# refusals: decided on the host, nothing is launched
# ---------------------------------------------------------------------------------------------------


def test_out_of_range_depth_counts_are_refused_before_any_launch():
    from lab4d_amd import _lib, render_utils as RU
    M, N = 1, 2
    g = RC.gen(7)
    hxy = torch.cat([torch.rand(M, N, 2, generator=g) * 64, torch.ones(M, N, 1)], -1).to(DEV)
    Kinv = torch.linalg.inv(torch.tensor([[64.0, 0, 32], [0, 64, 32], [0, 0, 1]]))[None].contiguous().to(DEV)
    nf = torch.tensor([[0.4, 0.8]], device=DEV)
    _lib.PROF = {}
    try:
        for D in (257, 0):
            fd = {"density": torch.rand(M, N, D, 1, device=DEV), "rgb": torch.rand(M, N, D, 3, device=DEV), "vis": torch.rand(M, N, D, 1, device=DEV)}
            fd["density_fg"] = fd["density"]
            deltas = torch.rand(M, N, D, 1, device=DEV) * 0.02
            with pytest.raises(RuntimeError, match="composite_forward"):
                RU.render_pixel(fd, deltas)
            # the entry points themselves, with every buffer large enough for the D they are told: the outputs keep their fill
            fl, gf = _lib.FieldList(), _lib.FieldGrads()
            fl.n_fields = gf.n_fields = 0
            outs = [torch.full((M, N, max(D, 1)), FILL, device=DEV) for _ in range(2)] + [torch.full((M, N, 1), FILL, device=DEV)]
            with pytest.raises(RuntimeError, match="composite_forward"):
                _lib.call("composite_forward", fd["density"], deltas, fl, None, None, None, M * N, D, *outs, None, None, None, None, None)
            gouts = [torch.full((M, N, max(D, 1), 1), FILL, device=DEV) for _ in range(2)]
            with pytest.raises(RuntimeError, match="composite_backward"):
                _lib.call("composite_backward", fd["density"], deltas, fl, None, None, None, M * N, D, outs[2], None, None, None, None,
                          *gouts, gf, None, None, None)
            torch.cuda.synchronize()
            assert all(bool((t == FILL).all()) for t in outs + gouts)
        with pytest.raises(RuntimeError, match="ray_samples_forward"):
            RU.sample_cam_rays(hxy, Kinv, nf, n_depth=1)
        routs = [torch.full((M, N, 1, c), FILL, device=DEV) for c in (3, 3, 1, 1)]
        with pytest.raises(RuntimeError, match="ray_samples_forward"):
            _lib.call("ray_samples_forward", hxy, Kinv, nf, None, None, None, M, N, 1, *routs, None, None)
        gK = torch.full((M, 3, 3), FILL, device=DEV)
        with pytest.raises(RuntimeError, match="ray_samples_backward"):
            _lib.call("ray_samples_backward", hxy, Kinv, nf, None, None, None, M, N, 1, routs[0], routs[1], routs[2], None, None, gK, None, None)
        torch.cuda.synchronize()
        assert all(bool((t == FILL).all()) for t in routs + [gK])
        assert _lib.prof_summary() == {}, "a refused call launched nothing: it has no place in the per-kernel profile"
    finally:
        _lib.PROF = None
