"""The multi-target blend entries (lab4d_skin_blend_forward_multi / _backward_multi, csrc/skinning.hip k_blend_*_multi) against the path they
replace: lab4d_skin_blend_forward once per target, lab4d_skin_blend_backward for target 0 followed by lab4d_skin_blend_backward_acc for target 1.

Forward outputs must be the same bits.  The adjoint sums the targets' dL/dp ahead of the softmax adjoint, where the two-launch path adds two
finished g_xyz / g_raw, so those two agree to rounding and not bit for bit; like the per-frame outputs (atomics in both paths) they are held
the way tests/test_gpu_skinning_kernels.py holds these tensors, with the two-launch path in the place of the float32 reference: the relative
L2 distance from the float64 truth of tests/skinning_cases.py is at most bound(e) = max(1e-4, 2 e), e being the two-launch path's own distance
on the same inputs (raypath_cases.bound: that file's floor and factor).  The inputs away from the float64 cases -- an exact softmax tie,
antipodal target quaternions, large logits -- sit ON the discontinuities the float64 cases keep clear of: there the forward must still be the
same bits and the two adjoints, which take the same branches, are held to 1e-4 of each other, the same floor."""
import ctypes

import pytest
import torch

import skinning_cases as SC
from lab4d_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = -7.0
CASES = [SC._case(2, spf, 2 * spf, B) for B in SC.BONES for spf in (256, 768)]


def _L():
    from lab4d_amd import _lib as L
    return L


def call(name, *a):
    _L().call(name, *a)
    torch.cuda.synchronize()


def full(*shape):
    return torch.full(shape, FILL, device=DEV)


def ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def targets_of(case):
    """The case's inputs (CPU) for two targets: target 0 as tests/skinning_cases.py draws it, target 1 with the se3 tables of the frames in
    reverse order and a cotangent of its own.  entropy / delta_skin belong to the skin weights: their cotangents go in once."""
    inp = SC.blend_inputs(case)
    zero = torch.zeros_like(inp["w_ent"])
    t1 = dict(inp, se3_r=inp["se3_r"].flip(0).contiguous(), se3_d=inp["se3_d"].flip(0).contiguous(),
              w_out=torch.randn(case.S, 3, generator=SC.gen(77 + case.spf + case.B)), w_ent=zero, w_dskin=zero)
    return [inp, t1]


def dev(inp):
    return {k: v.to(DEV).contiguous() for k, v in inp.items() if isinstance(v, torch.Tensor)}


def run_single(case, tg, ent_with=0):
    """One forward launch per target; backward for target 0, backward_acc for target 1.  tg: device inputs per target."""
    S, M, B, spf = case.S, case.M, case.B, case.spf
    D = tg[0]
    tab = (D["xyz"], D["art_r"], D["art_d"], D["gauss"], D["raw"])
    o = {"ent": full(S), "dskin": full(S), "g_xyz": full(S, 3), "g_raw": full(S, B)}
    n = int(_L().lib().lab4d_skin_blend_backward_workspace_floats(S, spf, M, B, 1))
    par = []
    for t, X in enumerate(tg):
        o["out%d" % t] = full(S, 3)
        call("skin_blend_forward", *tab, X["se3_r"], X["se3_d"], S, spf, M, B, o["out%d" % t], o["ent"] if t == 0 else None,
             o["dskin"] if t == 0 else None, full(M * B * 12))
        o["g_se3_%d" % t] = torch.zeros(M, B, 8, device=DEV)
        p = [full(M, B, 4), full(M, B, 4), torch.zeros(B, 3, device=DEV)]
        call("skin_blend_backward_acc", *tab, X["se3_r"], X["se3_d"], X["w_out"], D["w_ent"] if t == ent_with else None,
             D["w_dskin"] if t == ent_with else None, S, spf, M, B, o["g_xyz"], o["g_raw"], o["g_se3_%d" % t], *p, full(n), 1 if t else 0)
        par.append(p)
    o["g_art_r"], o["g_art_d"], o["g_gauss"] = [par[0][i] + par[1][i] for i in range(3)]
    return o


def run_multi(case, tg):
    S, M, B, spf = case.S, case.M, case.B, case.spf
    D = tg[0]
    tab = (D["xyz"], D["art_r"], D["art_d"], D["gauss"], D["raw"], 2, ptrs([X["se3_r"] for X in tg]), ptrs([X["se3_d"] for X in tg]))
    o = {"ent": full(S), "dskin": full(S), "g_xyz": full(S, 3), "g_raw": full(S, B), "out0": full(S, 3), "out1": full(S, 3),
         "g_se3_0": torch.zeros(M, B, 8, device=DEV), "g_se3_1": torch.zeros(M, B, 8, device=DEV),
         "g_art_r": full(M, B, 4), "g_art_d": full(M, B, 4), "g_gauss": torch.zeros(B, 3, device=DEV)}
    call("skin_blend_forward_multi", *tab, S, spf, M, B, ptrs([o["out0"], o["out1"]]), o["ent"], o["dskin"], full(M * B * 12))
    n = int(_L().lib().lab4d_skin_blend_backward_workspace_floats(S, spf, M, B, 1))
    assert n == M * B * 34
    call("skin_blend_backward_multi", *tab, ptrs([X["w_out"] for X in tg]), D["w_ent"], D["w_dskin"], S, spf, M, B, o["g_xyz"], o["g_raw"],
         ptrs([o["g_se3_0"], o["g_se3_1"]]), o["g_art_r"], o["g_art_d"], o["g_gauss"], full(n))
    return o


FORWARD = ("out0", "out1", "ent", "dskin")
ADJOINT = ("g_xyz", "g_raw", "g_se3_0", "g_se3_1", "g_art_r", "g_art_d", "g_gauss")


def truth_of(tgs):
    """float64 truth of the two-target adjoint: per-target se3 gradients, everything else summed over the targets."""
    r = [SC.run_blend(t, torch.float64)[0] for t in tgs]
    t = {k: r[0][k] + r[1][k] for k in ("g_xyz", "g_raw", "g_art_r", "g_art_d", "g_gauss")}
    t["g_se3_0"], t["g_se3_1"] = r[0]["g_se3"], r[1]["g_se3"]
    return t


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_multi_equals_two_single_target_launches(case):
    tgs = targets_of(case)
    tg = [dev(t) for t in tgs]
    one, two = run_single(case, tg), run_multi(case, tg)
    for k in FORWARD:
        assert torch.equal(one[k], two[k]), k
        assert bool((two[k] != FILL).all()), k
    truth = truth_of(tgs)
    fig = {}
    for k in ADJOINT:
        e1, e2 = SC.rel_l2(one[k].reshape(truth[k].shape), truth[k]), SC.rel_l2(two[k].reshape(truth[k].shape), truth[k])
        fig[k] = (e2, e1)
        print("%s %s: e_multi %.3e e_single %.3e" % (case.name, k, e2, e1))
    bad = {k: v for k, v in fig.items() if not v[0] <= SC.bound(v[1])}
    assert not bad, bad
    # per-frame tensors: the bound on every frame row by itself, as tests/skinning_cases.verdict holds them
    for k in ("g_se3_0", "g_se3_1", "g_art_r", "g_art_d"):
        for m in range(case.M):
            e1, e2 = SC.rel_l2(one[k].reshape(truth[k].shape)[m], truth[k][m]), SC.rel_l2(two[k].reshape(truth[k].shape)[m], truth[k][m])
            assert e2 <= SC.bound(e1), (k, m, e2, e1)


def _edge_inputs(case, kind):
    """The case's inputs moved ONTO a discontinuity or to an extreme (CPU, float32, new tensors: the cached inputs are left alone)."""
    tgs = [dict(t) for t in targets_of(case)]
    inp = tgs[0]
    if kind == "tie":  # bone i becomes a copy of the most often nearest bone j (tables, scales, logits): every sample nearest to j sits at the same
        # distance from both, in any arithmetic -- skin_i == skin_j bit for bit in every kernel, so all of them take the first of the two
        # as the anchor (a tie to rounding only would let kernels that contract their multiply-adds differently pick different anchors,
        # and the entropy adjoint is discontinuous in the anchor).  The targets' tables of i and j stay different.
        best = SC._skin64(inp).argmax(-1)
        j = int(best.bincount(minlength=case.B).argmax())
        i = (j + 1) % case.B
        raw = inp["raw"].clone()
        raw[:, i] = raw[:, j]
        art_r, art_d, gauss = inp["art_r"].clone(), inp["art_d"].clone(), inp["gauss"].clone()
        art_r[:, i], art_d[:, i], gauss[i] = art_r[:, j], art_d[:, j], gauss[j]
        for t in tgs:
            t.update(raw=raw, art_r=art_r, art_d=art_d, gauss=gauss)
        skin = SC._skin64(tgs[0])
        tied = (skin[:, i] == skin[:, j]) & (skin.max(-1)[0] == skin[:, j])
        assert int(tied.sum()) >= 8, "samples whose two best bones tie exactly"
    elif kind == "antipodal":  # target 1's tables are target 0's negated: the same transforms from the other hemisphere
        tgs[1]["se3_r"], tgs[1]["se3_d"] = -inp["se3_r"], -inp["se3_d"]
    elif kind == "large":  # logits in the hundreds: one weight is 1 and the others underflow to 0 in the softmax
        for t in tgs:
            t["raw"] = inp["raw"] * 2000
    elif kind == "same":  # both targets blend to the same tables
        tgs[1]["se3_r"], tgs[1]["se3_d"] = inp["se3_r"], inp["se3_d"]
    return tgs


@pytest.mark.parametrize("kind", ["tie", "antipodal", "large", "same"])
def test_edges_multi_equals_two_single_target_launches(kind):
    case = SC._case(2, 256, 512, 25)
    tgs = _edge_inputs(case, kind)
    tg = [dev(t) for t in tgs]
    one, two = run_single(case, tg), run_multi(case, tg)
    for k in FORWARD:
        assert torch.equal(one[k], two[k]), (kind, k)
    if kind == "antipodal":  # q and -q are one transform
        assert torch.equal(two["out0"], two["out1"])
    for k in ADJOINT:
        assert bool(torch.isfinite(two[k]).all()), (kind, k)
        e = SC.rel_l2(two[k], one[k].double().cpu())
        print("%s %s: multi against two launches %.3e" % (kind, k, e))
        assert e <= 1e-4, (kind, k, e)
    if kind == "same":
        # identical tables: the single-target adjoint of the SUMMED cotangents
        S, M, B, spf = case.S, case.M, case.B, case.spf
        D = tg[0]
        o = {"g_xyz": full(S, 3), "g_raw": full(S, B), "g_se3": torch.zeros(M, B, 8, device=DEV), "g_art_r": full(M, B, 4), "g_art_d": full(M, B, 4),
             "g_gauss": torch.zeros(B, 3, device=DEV)}
        n = int(_L().lib().lab4d_skin_blend_backward_workspace_floats(S, spf, M, B, 1))
        call("skin_blend_backward", D["xyz"], D["art_r"], D["art_d"], D["gauss"], D["raw"], D["se3_r"], D["se3_d"], tg[0]["w_out"] + tg[1]["w_out"],
             D["w_ent"], D["w_dskin"], S, spf, M, B, o["g_xyz"], o["g_raw"], o["g_se3"], o["g_art_r"], o["g_art_d"], o["g_gauss"], full(n))
        # g_se3 is linear in the cotangent: the targets' two tensors add up to the single one (both scaled by the cotangents' shares)
        got = dict(two, g_se3=two["g_se3_0"] + two["g_se3_1"])
        for k in o:
            e = SC.rel_l2(got[k], o[k].double().cpu())
            print("same %s: multi against one launch on the summed cotangent %.3e" % (k, e))
            assert e <= 1e-4, (k, e)


def test_shapes_outside_the_dispatch_are_refused_without_a_launch_and_take_the_per_target_path():
    L = _L()
    from lab4d_amd import warping
    for S, spf, M, B, T in [(400, 200, 2, 25, 2), (512, 256, 2, 24, 2), (512, 256, 2, 25, 3), (512, 256, 2, 25, 1)]:
        assert not warping._blend_multi_shape(spf, B, T) and warping._blend_multi_work(S, spf, M, B, T, DEV) is None
    assert warping._blend_multi_shape(256, 18, 2)
    assert warping._blend_multi_work(512, 256, 2, 18, 2, DEV).numel() == 2 * 18 * 34
    case = SC._case(2, 256, 512, 25)
    tg = [dev(t) for t in targets_of(case)]
    D = tg[0]
    S, M, B = 400, 2, 25
    outs = {"out0": full(S, 3), "out1": full(S, 3), "ent": full(S), "dskin": full(S), "g_xyz": full(S, 3), "g_raw": full(S, B),
            "g_se3_0": full(M, B, 8), "g_se3_1": full(M, B, 8), "work": full(M * B * 34)}
    tab = (D["xyz"], D["art_r"], D["art_d"], D["gauss"], D["raw"], 2, ptrs([X["se3_r"] for X in tg]), ptrs([X["se3_d"] for X in tg]))
    L.PROF = {}
    try:
        with pytest.raises(RuntimeError, match="skin_blend_forward_multi"):
            L.call("skin_blend_forward_multi", *tab, S, 200, M, B, ptrs([outs["out0"], outs["out1"]]), outs["ent"], outs["dskin"], outs["work"])
        with pytest.raises(RuntimeError, match="skin_blend_backward_multi"):
            L.call("skin_blend_backward_multi", *tab, ptrs([X["w_out"] for X in tg]), D["w_ent"], D["w_dskin"], S, 200, M, B, outs["g_xyz"],
                   outs["g_raw"], ptrs([outs["g_se3_0"], outs["g_se3_1"]]), None, None, None, outs["work"])
        torch.cuda.synchronize()
        assert all(bool((v == FILL).all()) for v in outs.values()), "a refused call launched nothing: every output and the scratch keep their fill"
        # the autograd function at spf = 200: one launch per target, none of the multi-target entries
        x = D["xyz"][:S].clone().requires_grad_(True)
        flat = warping.SkinBlendMulti.apply(x, D["raw"][:S].contiguous(), D["art_r"], D["art_d"], D["gauss"], 200, tg[0]["se3_r"], tg[0]["se3_d"],
                                            tg[1]["se3_r"], tg[1]["se3_d"])
        (flat[0].sum() + flat[1].sum() + flat[2].sum()).backward()
        torch.cuda.synchronize()
        names = set(L.prof_summary())
        assert {"k_blend_fwd", "k_blend_bwd+gram"} <= names and not any("multi" in n for n in names), names
        L.PROF = {}
        x = D["xyz"].clone().requires_grad_(True)
        flat = warping.SkinBlendMulti.apply(x, D["raw"], D["art_r"], D["art_d"], D["gauss"], 256, tg[0]["se3_r"], tg[0]["se3_d"], tg[1]["se3_r"],
                                            tg[1]["se3_d"])
        (flat[0].sum() + flat[1].sum() + flat[2].sum()).backward()
        torch.cuda.synchronize()
        assert set(L.prof_summary()) == {"k_blend_fwd_multi", "k_blend_bwd_multi+gram"}, set(L.prof_summary())
    finally:
        L.PROF = None


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def test_forward_warp_pair_with_the_switch_on_and_off(monkeypatch):
    """skinning_warp_forward_multi at spf = 256 (the multi-target kernels) against the same call with warping.SKIN_BLEND_MULTI off: outputs bit
    for bit, gradients at the bound tests/test_gpu_skinning.py holds the shared evaluation to against separate warps (1e-5 of the maximum)."""
    from lab4d_amd import warping, mlp
    M, N, D = 2, 4, 64
    P0 = synthetic.make_weights(4)
    fr = synthetic.add_codes(synthetic.make_frames(5, M, 64), P0)
    g = torch.Generator().manual_seed(3)
    xyz = torch.randn(M, N, D, 3, generator=g) * 0.08
    ws = [torch.randn(M, N, D, 3, generator=g).to(DEV) for _ in range(2)]
    we = [torch.randn(M, N, D, 1, generator=g).to(DEV) for _ in range(2)]
    pkeys = ["warp.skinning_model.log_gauss", "warp.skinning_model.delta_field.linear_1.0.weight", "warp.skinning_model.delta_field.linear_final.weight"]

    def run(on):
        monkeypatch.setattr(warping, "SKIN_BLEND_MULTI", on)
        P = {k: (v.to(DEV).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(DEV)) for k, v in P0.items()}
        t_art = tuple(t.to(DEV).clone().requires_grad_(True) for t in fr["t_articulation"])
        nxt = tuple(t.to(DEV).flip(0).clone().requires_grad_(True) for t in fr["t_articulation"])
        rest = tuple(t.to(DEV).clone().requires_grad_(True) for t in fr["rest_articulation"])
        x = xyz.to(DEV).clone().requires_grad_(True)
        res = warping.skinning_warp_forward_multi(P, x, [nxt, t_art], rest, fr["t_embed_mean"].to(DEV), fr["code_skin"].to(DEV), mlp.PREC_F32)
        loss = sum((o * w).sum() + (aux["skin_entropy"] * e).sum() + (aux["delta_skin"] * e).sum() * 50 for (o, aux), w, e in zip(res, ws, we))
        gs = torch.autograd.grad(loss, [x, t_art[0], t_art[1], nxt[0], nxt[1], rest[0], rest[1]] + [P[k] for k in pkeys])
        return [o for o, _ in res] + [res[0][1]["skin_entropy"], res[0][1]["delta_skin"]], gs

    o1, g1 = run(True)
    o0, g0 = run(False)
    for a, b in zip(o1, o0):
        assert torch.equal(a, b)
    for a, b, n in zip(g1, g0, ["x", "t_r", "t_d", "n_r", "n_d", "rest_r", "rest_d"] + pkeys):
        print("switch on/off %s: %.3e" % (n, _rel(a, b)))
        assert _rel(a, b) < 1e-5, (n, _rel(a, b))


def test_training_graph_with_the_switch_on_and_off(monkeypatch):
    """render_train + losses + backward on synthetic frames with 4 rays x 64 depths = 256 samples per frame (the training fixtures under
    tests/golden/ have 30 per frame and never reach the multi-target kernels), warping.SKIN_BLEND_MULTI on and off: the profile shows which
    kernels ran, and every loss and parameter gradient agrees within 1e-4 of its maximum, the floor tests/test_gpu_field.py holds the
    training fixtures to."""
    from lab4d_amd import deformable as DF
    from lab4d_amd import mlp, warping
    L = _L()
    M, N, D, res = 2, 4, 64, 64
    P0 = synthetic.make_weights(3)
    g = torch.Generator().manual_seed(5)
    hxy = torch.cat([torch.rand(M, N, 2, generator=g) * res, torch.ones(M, N, 1)], -1)
    batch = synthetic.to_device(synthetic.make_targets(6, M, N, res, hxy), DEV)
    rng = synthetic.to_device({"eik_inds": torch.arange(1), "match_perm": torch.randperm(M * N * D, generator=g)}, DEV)

    def run(on):
        monkeypatch.setattr(warping, "SKIN_BLEND_MULTI", on)
        Pd = {k: (v.to(DEV).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(DEV)) for k, v in P0.items()}
        fr = synthetic.add_codes(synthetic.to_device(synthetic.make_frames(4, M, res), DEV), Pd)
        fr["feature"] = batch["feature"]
        L.PROF = {}
        try:
            out = DF.render_train(Pd, fr, hxy.to(DEV), rng, flow_thresh=float(res), n_depth=D, prec=mlp.PREC_F32)
            losses = DF.losses_fg(out, batch, res, DF.DEFAULT_LOSS_WT)
            sum(v for v in losses.values() if bool(torch.isfinite(v))).backward()
            torch.cuda.synchronize()
            names = set(L.prof_summary())
        finally:
            L.PROF = None
        return losses, {k: v.grad for k, v in Pd.items() if v.dtype.is_floating_point and v.grad is not None}, names

    l1, g1, n1 = run(True)
    l0, g0, n0 = run(False)
    assert {"k_blend_fwd_multi", "k_blend_bwd_multi+gram"} <= n1 and not any("multi" in n for n in n0), (n1, n0)
    assert set(l1) == set(l0) and set(g1) == set(g0) and len(g0) > 10
    for k in l0:
        assert bool(torch.isfinite(l1[k])) == bool(torch.isfinite(l0[k])), k
        if bool(torch.isfinite(l0[k])):
            assert _rel(l1[k], l0[k]) <= 1e-4, (k, _rel(l1[k], l0[k]))
    for k in g0:
        print("training graph switch on/off %s: %.3e" % (k, _rel(g1[k], g0[k])))
        assert _rel(g1[k], g0[k]) <= 1e-4, (k, _rel(g1[k], g0[k]))


# ---------------------------------------------------------------------------------------------------
# grid-stride passes: every block walks several tiles, of different frames
# ---------------------------------------------------------------------------------------------------


def _tiled_targets(case, with_truth=True):
    """Device inputs per target of a case of M = reps x PERIOD frames whose frames repeat with period PERIOD, and the float64 truth of its
    two-target adjoint, both tiled on the device from the period's (tests/test_gpu_skinning_kernels.py _tiled); g_gauss is reps x the period's."""
    pc = SC.period_case(case)
    reps = case.M // SC.PERIOD
    tgs = targets_of(pc)
    rep = lambda v: v.to(DEV).repeat(reps, *([1] * (v.dim() - 1))).contiguous()
    tg = [{k: (v.to(DEV).contiguous() if k == "gauss" else rep(v)) for k, v in t.items() if isinstance(v, torch.Tensor) and k not in ("frame", "w_bone")} for t in tgs]
    truth = {k: (v.to(DEV) * reps if k == "g_gauss" else rep(v)) for k, v in truth_of(tgs).items()} if with_truth else None
    return tg, truth


def _rel_dev(d, t):
    """Relative L2 distance from the float64 truth, on the device."""
    d, t = d.detach().reshape(t.shape).double(), t.double()
    n = float(t.norm())
    return float((d - t).norm()) / n if n > 0 else float((d - t).norm())


def test_grid_stride_every_block_walks_several_tiles_and_frames():
    """S = 524,800 = 2,050 frames of one tile: the 2,048 resident blocks of k_blend_bwd_multi<25,2> start a second tile, of another frame --
    the block sums are flushed to the first frame and start again, and the three LDS tiles are refilled behind the previous tile's readers.
    Multi against the two-launch path: forward bit for bit; the adjoints against the tiled float64 truth at bound(the two-launch path's own
    distance) -- over everything, then over the samples and the frames that only the second pass reaches, and frame by frame there."""
    case = SC.GRID_FUSED
    first = SC.CAPS["fused"] * 256
    assert case.S > first and case.spf == 256
    tg, truth = _tiled_targets(case)
    one, two = run_single(case, tg), run_multi(case, tg)
    for k in FORWARD:
        assert torch.equal(one[k], two[k]), k
    for k in ADJOINT:
        views = {"all": slice(None)}
        if k != "g_gauss":
            views["beyond"] = slice(first, None) if k in ("g_xyz", "g_raw") else slice(first // case.spf, None)
        if k not in ("g_xyz", "g_raw", "g_gauss"):
            views.update({"frame %d" % m: slice(m, m + 1) for m in range(first // case.spf, case.M)})
        for what, rows in views.items():
            t = truth[k][rows]
            e1, e2 = _rel_dev(one[k].reshape(truth[k].shape)[rows], t), _rel_dev(two[k].reshape(truth[k].shape)[rows], t)
            print("grid %s %s: e_multi %.3e e_single %.3e" % (k, what, e2, e1))
            assert e2 <= SC.bound(e1), (k, what, e2, e1)


def test_grid_stride_forward_second_pass():
    """S = 2,099,200 > 8,192 blocks x 256: k_blend_fwd_multi<18,2> on its second pass, bit for bit the per-target launches."""
    case = SC.BlendCase("grid_fwd_multi", 8200, 256, 8200 * 256, 18)
    first = SC.CAPS["wide"] * 256
    assert case.S > first
    tg, _ = _tiled_targets(case, with_truth=False)
    S, M, B, spf = case.S, case.M, case.B, case.spf
    D = tg[0]
    o = {k: full(S, 3) for k in ("out0", "out1", "one0", "one1")}
    o.update({k: full(S) for k in ("ent", "dskin", "one_ent", "one_dskin")})
    call("skin_blend_forward_multi", D["xyz"], D["art_r"], D["art_d"], D["gauss"], D["raw"], 2, ptrs([X["se3_r"] for X in tg]),
         ptrs([X["se3_d"] for X in tg]), S, spf, M, B, ptrs([o["out0"], o["out1"]]), o["ent"], o["dskin"], full(M * B * 12))
    for t, X in enumerate(tg):
        call("skin_blend_forward", D["xyz"], D["art_r"], D["art_d"], D["gauss"], D["raw"], X["se3_r"], X["se3_d"], S, spf, M, B, o["one%d" % t],
             o["one_ent"] if t == 0 else None, o["one_dskin"] if t == 0 else None, full(M * B * 12))
    for a, b in (("out0", "one0"), ("out1", "one1"), ("ent", "one_ent"), ("dskin", "one_dskin")):
        assert torch.equal(o[a], o[b]), a
        assert bool((o[a][first:] != FILL).all()), a
