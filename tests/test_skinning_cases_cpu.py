"""The references tests/test_gpu_skinning_kernels.py holds the device to, checked without a GPU: for every small case the float64 truth is
finite and non-zero where the device writes, the float32 reference sits within E_REF_MAX of it (so max(1e-4, 2 e_ref) is 1e-4 throughout);
the inputs keep the arg-max anchor, the ReLU, the hemisphere sign and the nearest centre away from rounding on EVERY sample (nothing is
excluded from any comparison); a census pins the kernel instantiations the case lists reach, with the dispatch conditions it assumes read
from csrc/skinning.hip; and synthetic perturbations of a truth show that the metric sees the faults it is there for."""
import os
import re

import pytest
import torch

import skinning_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXCLUDED_SHARE_ALLOWED = 0.0
ALL_BLEND = SC.BLEND_CASES + [SC.period_case(SC.GRID_FUSED), SC.period_case(SC.GRID_UNFUSED)]


def _held(truth, ref32, what, nonzero=True):
    worst = 0.0
    for k, t in truth.items():
        assert bool(torch.isfinite(t).all()), (what, k)
        assert t.dtype == torch.float64 and ref32[k].dtype == torch.float32 and ref32[k].shape == t.shape, (what, k)
        if nonzero:
            assert float(t.abs().max()) > 0, (what, k)
        e = SC.rel_l2(ref32[k], t)
        assert e <= SC.E_REF_MAX, "%s %s: the float32 reference is %.2e from the float64 reference" % (what, k, e)
        worst = max(worst, e)
    assert SC.bound(worst) == 1e-4
    return worst


@pytest.mark.parametrize("case", ALL_BLEND, ids=lambda c: c.name)
def test_blend_and_bone_reference_error(case):
    truth, ref32, _, _ = SC.blend_reference(case)
    assert set(truth) == {"out", "ent", "dskin", "g_xyz", "g_raw", "g_se3", "g_art_r", "g_art_d", "g_gauss"}
    _held(truth, ref32, case.name)
    bt, br = SC.bone_reference(case)
    assert set(bt) == {"xyz_bone", "g_xyz", "g_art_r", "g_art_d", "g_gauss", "aff", "G"}
    _held(bt, br, case.name + " bone")
    # every frame that holds a sample receives a gradient; per-sample tensors are non-zero on every row
    frames = int(SC.blend_inputs(case)["frame"].max()) + 1
    for t in (truth["g_se3"], truth["g_art_r"], truth["g_art_d"], bt["g_art_r"], bt["G"], bt["aff"]):
        assert bool((t[:frames].reshape(frames, -1).abs().max(-1)[0] > 0).all())
    for t in (truth["out"], truth["g_xyz"], truth["g_raw"], bt["xyz_bone"], bt["g_xyz"]):
        assert bool((t.reshape(case.S, -1).abs().max(-1)[0] > 0).all())
    assert bool((truth["ent"] > 0).all()) and bool((truth["dskin"] > 0).all())


@pytest.mark.parametrize("case", ALL_BLEND, ids=lambda c: c.name)
def test_blend_inputs_keep_every_discontinuity_away_from_rounding(case):
    truth, ref32, a64, a32 = SC.blend_reference(case)
    inp = SC.blend_inputs(case)
    excluded = torch.zeros(case.S, dtype=torch.bool)
    # anchor
    top = a64["skin"].topk(2, -1)[0]
    excluded |= (top[:, 0] - top[:, 1]) < SC.ANCHOR_MARGIN
    excluded |= a64["anchor"] != a32["anchor"]
    # ReLU
    raw = inp["raw"]
    other = torch.arange(case.B) != SC.ZERO_COLUMN
    assert bool((raw[:, SC.ZERO_COLUMN] == 0).all())
    excluded |= (raw[:, other].abs() < SC.RELU_MARGIN).any(-1)
    for r in (truth, ref32):
        assert bool((r["g_raw"][:, SC.ZERO_COLUMN] == 0).all()), "raw == 0 is not > 0: no gradient"
        assert bool((r["g_raw"][raw < 0] == 0).all()) and bool((r["g_raw"][raw > 0] != 0).all())
    assert bool((raw > 0).any()) and bool((raw < 0).any())
    # hemisphere
    excluded |= (a64["hemi_dot"].abs() < SC.HEMI_MARGIN).any(-1)
    assert bool(((a64["hemi_dot"] > 0) == (a32["hemi_dot"] > 0)).all())
    assert float((a64["hemi_dot"] < 0).double().mean()) >= 0.2, "at least 20% of the (sample, bone) pairs take the sign -1"
    flipped = (inp["se3_r"][..., 0] < 0).float().mean()
    assert 0.3 <= float(flipped) <= 0.5
    assert float(excluded.double().mean()) <= EXCLUDED_SHARE_ALLOWED, "no sample is excluded anywhere"
    # the tables are what they claim: unit rotations, points inside frames
    assert float((inp["se3_r"].norm(dim=-1) - 1).abs().max()) < 1e-6 and float((inp["art_r"].norm(dim=-1) - 1).abs().max()) < 1e-6
    assert int(inp["frame"].max()) < case.M and case.S <= case.M * case.spf


def test_seed_that_needed_redrawing_is_covered():
    """(5,256,25) is the shape whose plain draw sat 1.2e-5 from an anchor tie: the redraw loop leaves the margin there too."""
    case = SC._case(5, 256, 5 * 256, 25)
    _, _, a64, a32 = SC.blend_reference(case)
    top = a64["skin"].topk(2, -1)[0]
    assert float((top[:, 0] - top[:, 1]).min()) >= SC.ANCHOR_MARGIN and bool((a64["anchor"] == a32["anchor"]).all())


@pytest.mark.parametrize("CA,CB", SC.GRAM_PAIRS)
def test_gram_reference_error(CA, CB):
    for spf in SC.GRAM_SPF:
        truth, ref32 = SC.gram_reference(CA, CB, spf)
        _held({"out": truth}, {"out": ref32}, "gram %dx%d spf %d" % (CA, CB, spf))
        inp = SC.gram_inputs(CA, CB, spf)
        S = SC.gram_S(spf)
        assert inp["A"].shape == (S, CA) and inp["Bm"].shape == (S, CB) and S < SC.GRAM_M * spf
        assert float(inp["prefill"].abs().min()) > 0
        frames = (S + spf - 1) // spf
        assert frames == (SC.GRAM_M if spf > 1 else 2), "a ragged last frame (spf = 1: an empty one)"
        added = (truth - inp["prefill"].double()).reshape(SC.GRAM_M, -1).abs().max(-1)[0]
        assert bool((added[:frames] > 0).all()) and bool((added[frames:] == 0).all())


@pytest.mark.parametrize("S,B", SC.GAUSS_CASES + [SC.GRID_GAUSS[2:0:-1]])
def test_gauss_reference_error_and_margins(S, B):
    truth, ref32 = SC.gauss_reference(S, B)
    _held(truth, ref32, "gauss s%d b%d" % (S, B))
    inp = SC.gauss_inputs(S, B)
    d = SC._centre_dist(inp["xyz"], inp["centres"]).topk(2, -1, largest=False)[0]
    assert float(d[:, 0].max()) <= 0.03, "within 0.03 of some centre"
    excluded = (d[:, 1] - d[:, 0]) < SC.CENTRE_GAP
    assert float(excluded.double().mean()) <= EXCLUDED_SHARE_ALLOWED
    assert float(truth["out"].min()) > 1e-3 * float(truth["out"].max()), "no value near underflow"
    assert bool((truth["g_xyz"].abs().max(-1)[0] > 0).all())


# ---------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------


def _census():
    ks = set()
    for c in SC.BLEND_CASES:
        ks |= SC.reached("bone_coords_forward", B=c.B, spf=c.spf)
        ks |= SC.reached("bone_coords_backward", B=c.B, spf=c.spf, params=False)
        ks |= SC.reached("bone_coords_backward", B=c.B, spf=c.spf, params=True)
        ks |= SC.reached("gram_per_frame", CB=4) | SC.reached("bone_params_from_gram") | SC.reached("bone_affine")
        if c.spf % 256 == 0:
            ks |= SC.reached("bone_coords_backward_gram", B=c.B, spf=c.spf)
        ks |= SC.reached("skin_blend_forward", B=c.B, spf=c.spf)
        for params, se3 in SC.ADJOINT_WAYS:
            ks |= SC.reached("skin_blend_backward", B=c.B, spf=c.spf, g_se3=se3, params=params)
    for c, se3 in SC.ACC_CASES:
        ks |= SC.reached("skin_blend_backward", B=c.B, spf=c.spf, g_se3=se3, params=True, accumulate=True)
    for _, CB in SC.GRAM_PAIRS:
        ks |= SC.reached("gram_per_frame", CB=CB)
    ks |= SC.reached("gauss_density_forward") | SC.reached("gauss_density_backward")
    return ks


def test_census_of_the_kernel_instantiations_the_cases_reach():
    assert _census() == SC.every_instantiation()
    assert len(SC.every_instantiation()) == 9 + 2 * (2 + 6 + 4 + 2)
    shapes = {(c.M, c.spf, c.S) for c in SC.BLEND_CASES}
    assert shapes == {(1, 1, 1), (2, 63, 126), (3, 100, 257), (1, 256, 255), (1, 256, 1), (2, 256, 512), (3, 256, 700), (2, 512, 1024)}
    for B in SC.BONES:
        assert {(c.M, c.spf, c.S) for c in SC.BLEND_CASES if c.B == B} == shapes
    assert len(SC.ADJOINT_WAYS) == 4 and set(SC.ADJOINT_WAYS) == {(True, True), (True, False), (False, True), (False, False)}
    # what the shapes are there for
    assert any(1 < c.spf < 256 and c.S > c.spf for c in SC.BLEND_CASES), "a frame edge inside a tile"
    assert any(c.S < c.M * c.spf and c.S % 256 == 1 and c.spf % 256 for c in SC.BLEND_CASES), "non-uniform, last tile of one sample"
    assert any(c.spf % 256 == 0 and c.S % 256 not in (0, 1, 255) and c.S > 256 for c in SC.BLEND_CASES), "uniform, ragged last tile"
    assert any(c.spf == 512 and c.S == c.M * 512 for c in SC.BLEND_CASES), "a frame spans two tiles"
    # accumulate: non-uniform, fused and uniform-unfused for each bone count
    acc = {(c.B, c.spf % 256 == 0, c.spf % 256 == 0 and se3) for c, se3 in SC.ACC_CASES}
    assert acc == {(B, u, f) for B in SC.BONES for u, f in [(False, False), (True, True), (True, False)]}
    assert {c.spf % 256 == 0 for c in SC.UNALIGNED_CASES} == {True, False} and {c.spf % 256 == 0 for c in SC.NULL_CASES} == {True, False}
    assert all(c.S % 256 for c in SC.UNALIGNED_CASES), "a partial tile on the scalar branch of RowTile as well"
    # gram_per_frame
    assert set(SC.GRAM_PAIRS) == {(75, 4), (54, 4), (25, 8), (18, 8), (25, 10), (18, 10), (80, 8), (1, 1), (40, 16), (7, 3)}
    assert set(SC.GRAM_SPF) == {1, 127, 128, 129, 1024, 1025} and SC.GRAM_M == 3
    assert [SC.gram_S(s) for s in (1, 127, 1025)] == [2, 376, 3070]
    assert all(CA <= 80 and CB <= 16 and CA * CB <= 640 for CA, CB in SC.GRAM_PAIRS)
    # grid-stride second passes
    f, u = SC.GRID_FUSED, SC.GRID_UNFUSED
    assert (f.M, f.spf, f.S, f.B) == (2050, 256, 524800, 25) and (u.M, u.spf, u.S, u.B) == (21000, 100, 2100000, 18)
    assert f.S > SC.CAPS["fused"] * 256 and (SC.CAPS["fused"] * 256) % (SC.PERIOD * f.spf) != 0
    assert u.S > SC.CAPS["wide"] * 256 and (SC.CAPS["wide"] * 256) % (SC.PERIOD * u.spf) != 0
    S, B, per = SC.GRID_GAUSS
    assert S > SC.CAPS["wide"] * 256 > SC.CAPS["gauss_bwd"] * 256 and S % per == 0 and (SC.CAPS["wide"] * 256) % per != 0
    assert (SC.CAPS["gauss_bwd"] * 256) % per != 0
    assert f.M % SC.PERIOD == 0 and u.M % SC.PERIOD == 0


def test_the_dispatch_conditions_the_census_assumes_are_the_source_s():
    src = open(os.path.join(ROOT, "lab4d_amd", "csrc", "skinning.hip")).read()

    def body(name):
        m = re.search(r'extern "C" int lab4d_%s\([^;{]*\)\s*\{.*?\n}\n' % name, src, re.S)  # the definition, not a declaration
        assert m, name
        return m.group(0)

    for name, kernel in [("bone_coords_forward", "k_bone_fwd"), ("skin_blend_forward", "k_blend_fwd")]:
        b = body(name)
        assert re.search(r"if \(spf %% 256 == 0\) \{ SKIN_DISPATCH\(B, hipLaunchKernelGGL\(\(%s<NB, true>\), dim3\(grid_1d\(S, 256, 8192\)\)" % kernel, b), name
        assert re.search(r"else \{ SKIN_DISPATCH\(B, hipLaunchKernelGGL\(\(%s<NB, false>\), dim3\(grid_1d\(S, 256, 8192\)\)" % kernel, b), name
    b = body("bone_coords_backward")
    assert re.search(r"if \(spf % 256 == 0\) \{ SKIN_DISPATCH\(B, hipLaunchKernelGGL\(\(k_bone_bwd_x<NB, true, false>\), dim3\(grid_1d\(S, 256, 8192\)\)", b)
    assert "k_bone_bwd_x<NB, false, false>" in b and "k_bone_bwd_p<NB>" in b
    assert b.index("parameter gradients must be requested together") < b.index("hipLaunchKernelGGL"), "refused before anything is launched"
    b = body("bone_coords_backward_gram")
    assert "spf % 256 == 0" in b and "grid_1d(S, 256, 2048)" in b and "k_bone_bwd_x<NB, true, true>" in b
    assert b.index("SKIN_REQUIRE_BONES") < b.index("zero_async")
    b = src[src.index("static bool blend_bwd_fused"):]
    assert "return fuse_env && spf % 256 == 0 && has_g_se3;" in b
    b = body("skin_blend_backward_acc")
    assert re.search(r"const int grid = grid_1d\(S, 256, 2048\);.*?BLEND_BWD\(true, true, grid\);\s*\} else if \(spf % 256 == 0\) \{\s*"
                     r"BLEND_BWD\(true, false, grid_1d\(S, 256, 8192\)\);\s*\} else \{\s*BLEND_BWD\(false, false, grid_1d\(S, 256, 8192\)\);", b, re.S)
    assert b.index("SKIN_REQUIRE_BONES") < b.index("hipLaunchKernelGGL")
    assert "grid_1d(S, 256, 8192)" in body("gauss_density_forward") and "grid_1d(S, 256, 1024)" in body("gauss_density_backward")
    b = body("gram_per_frame")
    assert "if (CB == 4)" in b and "else if (CB == 8)" in b and "else if (CB == 10)" in b and "const int chunk = 1024;" in b
    assert "constexpr int TS = 128;" in src
    assert "case 25:" in src and "case 18:" in src
    assert (SC.CAPS["fused"], SC.CAPS["wide"], SC.CAPS["gauss_bwd"]) == (2048, 8192, 1024)


# ---------------------------------------------------------------------------------------------------
# the metric sees it
# ---------------------------------------------------------------------------------------------------

SEEN_CASE = SC._case(3, 256, 700, 25)


def _sees(dev, truth, ref32, per_frame=False):
    ok, fig = SC.verdict(dev, truth, ref32, per_frame)
    ok0, _ = SC.verdict(ref32, truth, ref32, per_frame)
    assert ok0, "the float32 reference itself passes"
    assert not ok, fig
    return fig


def test_metric_sees_an_output_row_left_at_the_fill_value():
    truth, ref32, _, _ = SC.blend_reference(SEEN_CASE)
    for k in ("out", "g_xyz", "g_raw", "ent"):
        dev = ref32[k].clone()
        dev[699] = -7.0
        _sees(dev, truth[k], ref32[k])


def test_metric_sees_a_sample_dropped_from_one_frame_s_sum():
    """A 256-sample frame whose sum misses one sample: the per-frame Gram matrix, directly and as the se3 gradient of the blend."""
    CA, CB, spf = 25, 8, 1024
    inp = SC.gram_inputs(CA, CB, spf)
    truth, ref32 = SC.gram_reference(CA, CB, spf)
    A = inp["A"].clone()
    A[1024 + 300] = 0
    _sees(inp["prefill"] + SC.per_frame_gram(A, inp["Bm"], spf, SC.GRAM_M, torch.float32), truth, ref32)
    case = SEEN_CASE
    t, r, _, _ = SC.blend_reference(case)
    pert = {k: v.clone() for k, v in SC.blend_inputs(case).items()}
    for k in ("w_out", "w_ent", "w_dskin"):
        pert[k][256 + 17] = 0     # sample 17 of frame 1 contributes nothing
    dev, _ = SC.run_blend(pert, torch.float32)
    fig = _sees(dev["g_se3"], t["g_se3"], r["g_se3"], per_frame=True)
    assert fig["frames_over"] == 1


def test_metric_sees_one_flipped_hemisphere_sign():
    case = SEEN_CASE
    t, r, a64, _ = SC.blend_reference(case)
    p = a64["skin"].softmax(-1)
    second = p.topk(2, -1)
    s = int(second[0][:, 1].argmax())
    b = int(second[1][s, 1])
    signs = torch.where(a64["hemi_dot"] > 0, 1.0, -1.0)
    same, _ = SC.run_blend(SC.blend_inputs(case), torch.float32, signs=signs)
    assert SC.verdict(same["out"], t["out"], r["out"])[0], "the explicit-sign form reproduces the oracle"
    signs[s, b] *= -1
    dev, _ = SC.run_blend(SC.blend_inputs(case), torch.float32, signs=signs)
    assert int((dev["out"] != same["out"]).any(-1).sum()) == 1
    _sees(dev["out"], t["out"], r["out"])
    _sees(dev["g_se3"], t["g_se3"], r["g_se3"], per_frame=True)


def test_metric_sees_a_frame_row_taken_from_its_neighbour():
    """Among 2,050 frames one wrong row is 1/2050 of the squared norm; the per-frame bound does not dilute it."""
    t, r, _, _ = SC.blend_reference(SC.period_case(SC.GRID_FUSED))
    reps = SC.GRID_FUSED.M // SC.PERIOD
    for k in ("g_se3", "g_art_r", "g_art_d"):
        truth, ref32 = t[k].repeat(reps, 1, 1), r[k].repeat(reps, 1, 1)
        dev = ref32.clone()
        dev[2049] = ref32[2048]
        fig = _sees(dev, truth, ref32, per_frame=True)
        assert fig["frames_over"] == 1
