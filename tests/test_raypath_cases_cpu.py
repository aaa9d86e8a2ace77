"""The references tests/test_gpu_raypath.py holds the device to, checked without a GPU: for every case it parametrises over, the float64
truth is finite and the float32 oracle sits within E_REF_MAX of it (so max(1e-4, 2 e_ref) is 1e-4 throughout, with 2x room or more for
the reference itself); a census pins what the case lists reach, so an edited list fails here before a GPU run silently loses coverage."""
import pytest
import torch

import raypath_cases as RC


def _held(truth, ref32, what):
    worst = 0.0
    for k, t in truth.items():
        assert bool(torch.isfinite(t).all()), (what, k)
        assert t.dtype == torch.float64 and ref32[k].dtype == torch.float32 and ref32[k].shape == t.shape, (what, k)
        e = RC.rel_l2(ref32[k], t)
        assert e <= RC.E_REF_MAX, "%s %s: the float32 oracle is %.2e from the float64 oracle" % (what, k, e)
        worst = max(worst, e)
    assert RC.bound(worst) == RC.NORTH_STAR_TOL
    return worst


@pytest.mark.parametrize("case", RC.COMPOSITE_CASES, ids=lambda c: c.name)
def test_composite_reference_error(case):
    truth, ref32 = RC.composite_reference(case)
    _held(truth, ref32, case.name)
    # what the fused kernels emit is all there: the rendered channels, the gradient of every differentiable leaf
    keys = {"out.mask", "out.mask_fg", "out.rgb", "out.xyz_cam", "out.eikonal", "out.vis", "out.gauss_mask", "out.aux2", "out.aux5", "out.aux7",
            "grad.density", "grad.deltas", "grad.rgb", "grad.vis", "grad.gauss_density", "grad.eikonal", "grad.aux5"}
    keys |= {"out.flow", "out.feature", "grad.flow_uv", "grad.feature"} if case.train else {"out.normal", "grad.normal"}
    assert keys <= set(truth)


def test_degenerate_rays_are_what_they_claim():
    m, j = RC.BAD_RAY
    for case in RC.COMPOSITE_CASES:
        truth, _ = RC.composite_reference(case)
        inp = RC.composite_inputs(case)
        w, T = RC.O.compute_weights(inp["density"], inp["deltas"])
        if case.kind == "empty":
            assert float(truth["out.mask"][m, j]) == 0 and float(truth["out.gauss_mask"][m, j]) == 0
            assert float(truth["out.rgb"][m, j].abs().max()) == 0
        elif case.kind == "opaque":
            assert float(T[m, j, case.D // 4 - 1]) == 0, "float32 transmittance underflows to exactly 0 inside the opaque run"
            assert abs(float(truth["out.mask"][m, j]) - 1) < 1e-12
        elif case.kind == "noflow":
            assert float(truth["out.flow"][m, j].abs().max()) == 0 and float(truth["grad.flow_uv"][m, j].abs().max()) == 0
            assert float(truth["out.flow"].abs().min(-1)[0].max()) > 0  # (the other rays do have flow)


@pytest.mark.parametrize("D", RC.WEIGHTS_D)
def test_compute_weights_reference_error(D):
    truth, ref32 = RC.weights_reference(D)
    _held(truth, ref32, "weights_d%d" % D)
    assert float((truth["out.weights"].sum(-1) + truth["out.transmit"][..., -1] - 1).abs().max()) < 1e-12


@pytest.mark.parametrize("case", RC.RAY_CASES, ids=lambda c: c.name)
def test_ray_reference_error(case):
    truth, ref32 = RC.ray_reference(case)
    _held(truth, ref32, case.name)
    _held(*RC.cam_rays_reference(case), case.name + " unfused")
    assert torch.equal(truth["out.depth"].float(), ref32["out.depth"]), "both references integrate the same sample positions"
    qn = RC.ray_inputs(case)["cq"].norm(dim=-1)
    assert bool(((qn - 1).abs() < 1e-6).all()) == case.unit_q
    if not case.unit_q:
        assert bool(((qn - 1).abs() > 1e-3).all()) and float(qn.min()) >= 0.7 - 1e-6 and float(qn.max()) <= 1.3 + 1e-6


def test_census_of_what_the_cases_reach():
    cases = RC.COMPOSITE_CASES
    assert {(c.D + 63) // 64 for c in cases} == {1, 2, 3, 4}, "every NC the compositing kernels are instantiated for"
    assert {c.D for c in cases if c.kind == "plain" and c.train} >= {1, 2, 63, 64, 65, 128, 129, 192, 193, 256}
    assert {c.D for c in cases if not c.train} == {65, 192}
    for kind in RC.KINDS[1:]:
        assert {c.D for c in cases if c.kind == kind} == {65, 193}, kind
    assert {c.kind for c in cases} == set(RC.KINDS)
    assert any(c.M * c.N == 1 and c.D == 129 for c in cases)
    assert any((c.M * c.N) % 4 for c in cases), "a ray count that is no multiple of the 4 rays of a block"
    for case in cases + [RC.NULL_CASE]:
        fields = RC.composited_fields(case)
        assert len(fields) <= 16
        assert {RC.channel_class(C) for _, C, m in fields if m != 2} == {"divides64", "three", "generic"}, case.name
        assert {m for _, _, m in fields} == {0, 1, 2}, case.name
        assert {C for _, C, _ in fields} >= {2, 5, 7}, case.name
        if case.train:  # the LDS-atomic branch and the shuffle branch alternate across consecutive mode-0 fields
            cls = [RC.channel_class(C) for k, C, m in fields if m == 0]
            assert any(cls[i:i + 3] == ["generic", "divides64", "generic"] for i in range(len(cls))), (case.name, cls)
            names = [k for k, _, _ in fields]
            assert names.index("aux5") + 1 == names.index("feature") == names.index("aux7") - 1
    assert set(RC.WEIGHTS_D) == {1, 65, 192, 256}
    M, N, D = RC.GRID_STRIDE_COMPOSITE
    assert (M * N + 3) // 4 > 16384 and M * N > 65536
    M, N, D = RC.GRID_STRIDE_RAYS
    assert M * N * D > 8192 * 256
    rays = {(c.M, c.N, c.D, c.with_depth, c.unit_q) for c in RC.RAY_CASES}
    assert rays == {(1, 1, 2, False, True), (3, 63, 3, True, True), (2, 64, 63, False, False), (2, 65, 64, True, False),
                    (1, 129, 65, False, True), (2, 5, 129, True, False), (1, 300, 128, False, True)}
    assert (RC.NULL_CASE.D, RC.NULL_RAY_CASE.N) == (65, 65)


def test_sort_depth_cases_hold_the_two_special_rows():
    cases = RC.sort_depth_cases()
    assert {(a.shape[0], a.shape[1], b.shape[1]) for _, a, b in cases} == {(1, 1, 1), (257, 64, 1), (257, 1, 64), (300, 64, 16)}
    assert any(a.shape[0] > 3 and float(a[3].min()) == float(a[3].max()) == float(b[3].min()) == float(b[3].max()) for _, a, b in cases)
    assert any(b.shape[1] >= 8 and bool((b[5, 3:8] < b[5, 2:7]).all()) for _, a, b in cases)
