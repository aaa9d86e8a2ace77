"""GPU parity of the fused posenc+MLP chain kernels (forward, dgrad chain, wgrad) vs the CPU oracle.
fp32 path (v_mfma_f32_32x32x2_f32): rtol 1e-4 (north_star).  bf16 path: bf16 operand rounding through
up to 10 stacked layers -> compared at 5e-2 of the output scale (documented in DESIGN.md)."""
import pytest
import torch
import torch.nn.functional as F

from lab4d_amd import synthetic
from oracle import lab4d_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_err(a, b):
    a, b = a.detach().float().cpu(), b.detach().float()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def setup(seed, M, N, D):
    P = synthetic.make_weights(seed)
    fr = synthetic.add_codes(synthetic.make_frames(seed + 1, M, 64), P)
    g = torch.Generator().manual_seed(seed + 2)
    xyz = torch.randn(M, N, D, 3, generator=g) * 0.15
    return P, fr, xyz, g


def ref_net(name, P, fr, xyz, feat_ext=None):
    if name == "vis":
        return O.vis_field(P, xyz, fr["code_vis"])
    if name == "base":
        feat = O.cond_mlp(P, "basefield", O.pos_embedding(xyz, 10), fr["code_base"], D=8, final_act=True)
        return F.linear(feat, P["sdf.weight"], P["sdf.bias"]), feat
    if name == "feat":
        return O.base_mlp(P, "feature_field", O.pos_embedding(xyz, 6), D=5, final_act=False)
    if name == "skin":
        t = fr["t_embed"].reshape(-1, 1, 1, 128).expand(xyz.shape[:-1] + (128,))
        return O.cond_mlp(P, "warp.skinning_model.delta_field", torch.cat([xyz, t], -1), fr["code_skin"], D=2, final_act=False)
    if name == "color":
        cf = O.cond_mlp(P, "colorfield", O.pos_embedding(xyz, 12), fr["code_color"], D=2, final_act=True) + feat_ext
        a = fr["appr_code"].view(-1, 1, 1, 32).expand(xyz.shape[:-1] + (32,))
        h = F.relu(F.linear(torch.cat([cf, a], -1), P["rgb.0.weight"], P["rgb.0.bias"]))
        return F.linear(h, P["rgb.2.weight"], P["rgb.2.bias"])
    raise ValueError(name)


def dev_net(name, prec, P, fr, xyz, ext=None):
    from lab4d_amd import mlp
    M = xyz.shape[0]
    spf = xyz.shape[1] * xyz.shape[2]
    x = xyz.reshape(-1, xyz.shape[-1])
    if name == "vis":
        return mlp.run_chain(mlp.NET_VIS, prec, P, x, spf, conds={0: fr["code_vis"]})
    if name == "base":
        return mlp.run_chain(mlp.NET_FG_BASE, prec, P, x, spf, conds={0: fr["code_base"], 4: fr["code_base"]}, export_layer=8)
    if name == "feat":
        return mlp.run_chain(mlp.NET_FEAT, prec, P, x, spf)
    if name == "skin":
        return mlp.run_chain(mlp.NET_SKIN, prec, P, x, spf, conds={0: torch.cat([fr["t_embed"], fr["code_skin"]], -1)})
    if name == "color":
        return mlp.run_chain(mlp.NET_FG_COLOR, prec, P, x, spf, conds={0: fr["code_color"], 3: fr["appr_code"]}, ext=ext)
    raise ValueError(name)


GRAD_KEYS = {
    "vis": ["vis_mlp.basefield.linear_1.0.weight", "vis_mlp.basefield.linear_1.0.bias", "vis_mlp.basefield.linear_2.0.weight",
            "vis_mlp.basefield.linear_final.weight", "vis_mlp.basefield.linear_final.bias"],
    "base": ["basefield.linear_1.0.weight", "basefield.linear_3.0.weight", "basefield.linear_5.0.weight", "basefield.linear_5.0.bias",
             "basefield.linear_final.0.weight", "sdf.weight", "sdf.bias"],
    "feat": ["feature_field.linear_1.0.weight", "feature_field.linear_5.0.weight", "feature_field.linear_final.weight",
             "feature_field.linear_final.bias"],
    "skin": ["warp.skinning_model.delta_field.linear_1.0.weight", "warp.skinning_model.delta_field.linear_2.0.bias",
             "warp.skinning_model.delta_field.linear_final.weight"],
}
TOL = {0: (1e-4, 3e-4), 1: (6e-2, 3e-1)}  # precision -> (forward rel-to-max, gradient rel-to-max)


def cosine(a, b):
    a, b = a.detach().float().cpu().flatten(), b.detach().float().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("name,cin,shape", [("vis", 3, (2, 5, 16)), ("skin", 75, (2, 3, 24)), ("feat", 3, (2, 7, 8)), ("base", 3, (2, 9, 8)),
                                            ("vis", 3, (2, 16, 16)), ("base", 3, (3, 32, 8))])  # spf % 256 == 0: per-frame bias grads folded into wgrad
def test_chain_forward_backward(name, cin, shape, prec):
    M, N, D = shape
    P, fr, xyz, g = setup(3, M, N, D)
    if cin != 3:
        xyz = torch.randn(M, N, D, cin, generator=g) * 0.5
    wt = torch.randn(M * N * D, 1 if name in ("vis", "base") else (16 if name == "feat" else 25), generator=g)
    ftol, gtol = TOL[prec]
    keys = GRAD_KEYS[name]
    cond_keys = {"vis": ["code_vis"], "base": ["code_base"], "feat": [], "skin": ["t_embed", "code_skin"]}[name]

    def run(fn, dev):
        Pl = {k: (v.to(dev).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(dev)) for k, v in P.items()}
        frl = {k: (v.to(dev).clone().requires_grad_(True) if torch.is_tensor(v) and v.dtype.is_floating_point else synthetic.to_device(v, dev))
               for k, v in fr.items()}
        x = xyz.to(dev).clone().requires_grad_(True)
        out = fn(Pl, frl, x)
        if isinstance(out, tuple):
            out = out[0]
        out = out.reshape(-1, wt.shape[1])
        loss = (out * wt.to(dev)).sum()
        gs = torch.autograd.grad(loss, [x] + [Pl[k] for k in keys] + [frl[k] for k in cond_keys])
        return out, gs

    ro, rg = run(lambda P_, f_, x_: ref_net(name, P_, f_, x_), "cpu")
    do, dg = run(lambda P_, f_, x_: dev_net(name, prec, P_, f_, x_), DEV)
    measured = {"forward": rel_err(do, ro)}
    assert measured["forward"] < ftol, f"{name} forward rel err {rel_err(do, ro):.3e}"
    for nme, a, b in zip(["x"] + keys + cond_keys, dg, rg):
        e = measured["grad." + nme] = rel_err(a, b)
        assert e < gtol, f"{name} grad {nme} rel err {e:.3e}"
        assert cosine(a, b) > 0.98, f"{name} grad {nme} cosine {cosine(a, b):.4f}"
    if prec == 1:
        # round 5: the benched dtype is held per entry to max(1e-4, 2 x the committed MI355X measurement) like the fp32 path
        # (tests/parity_report.py); TOL[1] above stays as the a-priori ceiling
        from parity_report import check
        check("mlp_bf16_%s_%dx%dx%d" % (name, M, N, D), measured)


@pytest.mark.parametrize("prec", [0, 1])
def test_base_color_coupling(prec):
    """colorfield consumes the exported basefield feature; its gradient flows back into the base chain."""
    M, N, D = 2, 6, 8
    P, fr, xyz, g = setup(5, M, N, D)
    w_rgb = torch.randn(M * N * D, 3, generator=g)
    w_sdf = torch.randn(M * N * D, 1, generator=g)
    keys = ["basefield.linear_2.0.weight", "basefield.linear_final.0.weight", "colorfield.linear_1.0.weight", "rgb.0.weight", "rgb.2.weight", "rgb.0.bias"]
    ftol, gtol = TOL[prec]

    def run(dev):
        Pl = {k: (v.to(dev).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(dev)) for k, v in P.items()}
        frl = {k: (v.to(dev).clone().requires_grad_(True) if torch.is_tensor(v) and v.dtype.is_floating_point else synthetic.to_device(v, dev))
               for k, v in fr.items()}
        x = xyz.to(dev).clone().requires_grad_(True)
        if dev == "cpu":
            sdf, feat = ref_net("base", Pl, frl, x)
            rgb = ref_net("color", Pl, frl, x, feat_ext=feat)
        else:
            sdf, feat = dev_net("base", prec, Pl, frl, x)
            rgb = dev_net("color", prec, Pl, frl, x, ext=feat)
        loss = (rgb.reshape(-1, 3) * w_rgb.to(dev)).sum() + (sdf.reshape(-1, 1) * w_sdf.to(dev)).sum()
        gs = torch.autograd.grad(loss, [x, frl["appr_code"], frl["code_color"]] + [Pl[k] for k in keys])
        return sdf.reshape(-1, 1), rgb.reshape(-1, 3), gs

    rs, rr, rg = run("cpu")
    ds, dr, dg = run(DEV)
    assert rel_err(ds, rs) < ftol and rel_err(dr, rr) < ftol, (rel_err(ds, rs), rel_err(dr, rr))
    for nme, a, b in zip(["x", "appr", "code_color"] + keys, dg, rg):
        e = rel_err(a, b)
        assert e < gtol, f"grad {nme} rel err {e:.3e}"
        assert cosine(a, b) > 0.98, f"grad {nme} cosine {cosine(a, b):.4f}"


def test_posenc_annealing_window():
    from lab4d_amd import mlp
    M, N, D = 2, 4, 8
    P, fr, xyz, g = setup(7, M, N, D)
    alpha = 0.45
    w = torch.clamp(alpha * 10 - torch.arange(10.0), 0, 1)
    w = 0.5 * (1 + torch.cos(torch.pi * w + torch.pi))
    ref = O.cond_mlp(P, "vis_mlp.basefield", O.pos_embedding(xyz, 10, alpha), fr["code_vis"], D=2)
    Pd = synthetic.to_device(P, DEV)
    out = mlp.run_chain(mlp.NET_VIS, 0, Pd, xyz.reshape(-1, 3).to(DEV), N * D, conds={0: fr["code_vis"].to(DEV)}, freq_w=w.to(DEV))
    assert rel_err(out.reshape(ref.shape), ref) < 1e-4


def test_chain_full_size_linearity_property():
    """Size-independent property at benchmark scale (no oracle): the head is linear in the last-layer bias,
    f(b + e) - f(b) == e for every sample, and padded tail samples never leak."""
    from lab4d_amd import mlp
    P = synthetic.to_device(synthetic.make_weights(1), DEV)
    S = 128 * 512 + 37
    x = torch.rand(S, 3, device=DEV) * 0.3 - 0.15
    code = torch.zeros(1, 32, device=DEV)
    a = mlp.run_chain(mlp.NET_VIS, 1, P, x, S, conds={0: code})
    P2 = dict(P)
    P2["vis_mlp.basefield.linear_final.bias"] = P["vis_mlp.basefield.linear_final.bias"] + 0.5
    b = mlp.run_chain(mlp.NET_VIS, 1, P2, x, S, conds={0: code})
    assert a.shape == (S, 1)
    assert float(((b - a) - 0.5).abs().max()) < 1e-5


@pytest.mark.parametrize("prec,tol", [(0, 2e-3), (1, 0.35)])
def test_eikonal_value_and_weight_gradients(prec, tol):
    """(|d sdf/dx| - 1)^2 and its gradient wrt every basefield / sdf weight (second-order in the reference:
    torch_utils.compute_gradient with create_graph=True) through the primal + tangent-mode kernels."""
    from lab4d_amd import deformable as DF
    M, N, D = 2, 8, 8
    P, fr, xyz, g = setup(11, M, N, D)
    inds = torch.tensor([1, 5, 6, 12])
    w = torch.rand(M, N, D, 1, generator=g)
    keys = ["basefield.linear_1.0.weight", "basefield.linear_2.0.weight", "basefield.linear_5.0.weight", "basefield.linear_8.0.weight",
            "basefield.linear_final.0.weight", "sdf.weight"]

    def run(dev):
        Pl = {k: (v.to(dev).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(dev)) for k, v in P.items()}
        code = fr["code_base"].to(dev)
        if dev == "cpu":
            e = O.compute_eikonal(Pl, xyz, code, inds)
        else:
            e = DF.eikonal_subsample(Pl, xyz.to(dev), code, inds.to(dev), prec=prec)
        gs = torch.autograd.grad((e * w.to(dev)).sum(), [Pl[k] for k in keys])
        return e, gs

    re, rg = run("cpu")
    de, dg = run(DEV)
    assert rel_err(de, re) < (1e-3 if prec == 0 else 0.2), rel_err(de, re)
    for k, a, b in zip(keys, dg, rg):
        assert rel_err(a, b) < tol, f"{k}: {rel_err(a, b):.3e}"
        assert cosine(a, b) > 0.97, f"{k}: cosine {cosine(a, b):.4f}"


@pytest.mark.parametrize("prec", [0, 1])
def test_eikonal_primal_pattern_taken_from_the_field_pass(prec):
    """The eikonal term's primal pass on a drawn subset of the rays, with its ReLU sign words and stored embedding GATHERED from the training-mode
    basefield pass over all samples (mlp.run_chain(tap=...) -> mlp.eikonal_sdf(tap=...)) instead of recomputed: values bit for bit
    equal to the stand-alone form (the same kernel on the same inputs wrote the words that are gathered), weight gradients to rounding."""
    from lab4d_amd import deformable as DF, mlp
    M, N, D = 2, 6, 128
    P, fr, xyz, g = setup(21, M, N, D)
    inds = torch.tensor([0, 3, 4, 7, 10, 11])
    w = torch.rand(M, N, D, 1, generator=g).to(DEV)
    keys = [k for k in P if (k.startswith("basefield.linear_") or k == "sdf.weight") and k.endswith("weight")]
    Pl = {k: (v.to(DEV).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(DEV)) for k, v in P.items()}
    frd = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in fr.items()}
    x = xyz.to(DEV)

    def run(reuse):
        tap = {} if reuse else None
        DF.nerf_forward(Pl, x, frd, prec, with_color=False, tap=tap)  # the field pass over all samples (training mode: the weights require grad)
        assert (not reuse) or tap.get("emb") is not None
        e = DF.eikonal_subsample(Pl, x, frd["code_base"], inds.to(DEV), prec=prec, tap=tap)
        return e, torch.autograd.grad((e * w).sum(), [Pl[k] for k in keys])

    e1, g1 = run(True)
    e0, g0 = run(False)
    assert torch.equal(e1, e0)  # same sign words, same kernels
    for k, a, b in zip(keys, g1, g0):  # the weight-gradient kernels add their block partials atomically: equal up to the order of those additions
        assert rel_err(a, b.cpu()) < 1e-5, (k, rel_err(a, b.cpu()))


def test_eikonal_with_a_dead_layer_keeps_gradients_finite():
    """Every unit of the last hidden layer dead => d sdf/dx == 0 exactly: the loss is 1 per sample and its weight gradients are
    finite (the zero subgradient of the norm, as torch's norm backward takes it), not 0/0 spread through the wgrad GEMM."""
    from lab4d_amd import deformable as DF
    M, N, D = 2, 8, 8
    P, fr, xyz, g = setup(12, M, N, D)
    P = dict(P)
    P["basefield.linear_8.0.bias"] = torch.full_like(P["basefield.linear_8.0.bias"], -1e3)
    inds = torch.tensor([0, 3, 9, 15])
    keys = [k for k in P if k.startswith(("basefield.", "sdf.")) and P[k].dtype.is_floating_point and k.endswith(("weight", "bias"))]

    def run(dev):
        Pl = {k: (v.to(dev).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(dev)) for k, v in P.items()}
        e = (O.compute_eikonal(Pl, xyz, fr["code_base"], inds) if dev == "cpu"
             else DF.eikonal_subsample(Pl, xyz.to(dev), fr["code_base"].to(dev), inds.to(dev), prec=0))
        gs = torch.autograd.grad(e.sum(), [Pl[k] for k in keys], allow_unused=True)
        return e, gs

    re, rg = run("cpu")
    de, dg = run(DEV)
    assert float(re.reshape(-1, 8)[inds].min()) == 1.0 and float(re.sum()) == 8.0 * len(inds)  # 1 on the drawn rays, 0 elsewhere
    assert torch.equal(de.cpu(), re)
    for k, a, b in zip(keys, dg, rg):
        if a is None:
            continue
        assert bool(torch.isfinite(a).all()), k
        ref = torch.zeros_like(a.cpu()) if b is None else b
        assert float((a.cpu() - ref).abs().max()) == 0.0, k


def test_bg_field_forward_backward_matches_oracle():
    """Background NeRF (LAB4D_NET_BG_BASE / LAB4D_NET_BG_COLOR, the view direction as the second per-sample input) vs the
    oracle: rgb, density, and every gradient incl. d/d dir, fp32; bf16 stays close."""
    from lab4d_amd import deformable as DF, mlp, synthetic
    from oracle import lab4d_oracle as O
    M, N, D = 2, 37, 9   # 666 samples: exercises the padded tail tile
    P0 = synthetic.make_bg_weights(3)
    g = torch.Generator().manual_seed(12)
    xyz = torch.randn(M, N, D, 3, generator=g) * 0.3
    dirs = torch.randn(M, N, D, 3, generator=g)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    w, w1 = torch.randn(M, N, D, 3, generator=g), torch.randn(M, N, D, 1, generator=g)
    names = [k for k in P0 if (k.endswith("weight") or k.endswith("bias")) and not k.startswith("vis_mlp")]

    def run(dev, use_hip, prec=None):
        P = {k: v.to(dev).clone().requires_grad_(True) for k, v in P0.items()}
        x, d = xyz.to(dev).clone().requires_grad_(True), dirs.to(dev).clone().requires_grad_(True)
        inst = torch.zeros(M, dtype=torch.long, device=dev)
        codes = {"basefield": O.inst_code(P, "basefield", inst), "colorfield": O.inst_code(P, "colorfield", inst)}
        if use_hip:
            rgb, dens = DF.nerf_forward_bg(P, x, d, codes, prec)
        else:
            rgb, dens = O.nerf_forward(P, x, codes, cfg=O.BG_CFG, dir=d)
        loss = (rgb * w.to(dev)).sum() + (dens * w1.to(dev)).sum() * 0.01
        gs = torch.autograd.grad(loss, [x, d] + [P[n] for n in names])
        return rgb, dens, dict(zip(["xyz", "dir"] + names, gs))

    rr, rd, rg = run("cpu", False)
    hr, hd, hg = run(DEV, True, mlp.PREC_F32)
    rel = lambda a, b: float((a.detach().float().cpu() - b.detach().float()).abs().max() / (b.abs().max() + 1e-12))
    assert rel(hr, rr) < 1e-4 and rel(hd, rd) < 1e-4, (rel(hr, rr), rel(hd, rd))
    for k in rg:
        assert rel(hg[k], rg[k]) < 2e-3, f"grad {k}: {rel(hg[k], rg[k]):.3e}"
    br, bd_, _ = run(DEV, True, mlp.PREC_BF16)
    assert rel(br, rr) < 6e-2 and rel(bd_, rd) < 6e-2


@pytest.mark.parametrize("net_name", ["vis", "skin25", "skin18"])
def test_fused_narrow_backward_equals_the_stored_activation_path(net_name, monkeypatch):
    """Round 4: the <= 64-wide nets' backward as ONE kernel that recomputes the forward and forms every weight gradient in registers
    (lab4d_mlp_backward_fused) against the stored-activation path (training-mode forward + dgrad chain + one weight-gradient launch per layer),
    both bf16, same inputs: 3 frames of 320 samples, the last one cut short (S = 900: a ragged last tile), weights / biases / per-frame tables /
    points / affine table gradients in the L2 norm.  The two paths round the same places to bf16 (activations, dZ); they differ in the bias
    gradient's summation order, in the posenc Jacobian's partner (fp32 here, the stored bf16 embedding there) and in the point entering the
    affine table's gradient as hi + lo bf16 -- so close, not equal."""
    import os
    from lab4d_amd import mlp, warping
    if net_name == "vis" and os.environ.get("LAB4D_FUSED_VIS", "0") == "0":
        pytest.skip("the fused backward of the visibility net is opt-in (LAB4D_FUSED_VIS=1, read once by the library): measured slower than its stored-activation path")
    M, spf, S = 3, 320, 900
    nb = 18 if net_name == "skin18" else 25
    P0 = synthetic.make_weights(6, num_bones=nb)
    fr = synthetic.add_codes(synthetic.make_frames(7, M, 64, num_bones=nb), P0)
    g = torch.Generator().manual_seed(8)
    x0 = (torch.randn(S, 3, generator=g) * (0.15 if net_name == "vis" else 0.08)).to(DEV)
    cout = 1 if net_name == "vis" else nb
    w = torch.randn(S, cout, generator=g).to(DEV)
    q = "warp.skinning_model.delta_field."
    keys = GRAD_KEYS["vis"] if net_name == "vis" else ["warp.skinning_model.log_gauss", q + "linear_1.0.weight", q + "linear_1.0.bias", q + "linear_2.0.weight",
                                                      q + "linear_2.0.bias", q + "linear_final.weight", q + "linear_final.bias"]

    def run(fused):
        monkeypatch.setattr(mlp, "FUSED_NARROW_BWD", fused)
        P = {k: (v.to(DEV).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(DEV)) for k, v in P0.items()}
        x = x0.clone().requires_grad_(True)
        if net_name == "vis":
            code = fr["code_vis"].to(DEV).clone().requires_grad_(True)
            out = mlp.run_chain(mlp.NET_VIS, mlp.PREC_BF16, P, x, spf, conds={0: code})
            leaves = [x, code]
        else:
            art = tuple(t.to(DEV).clone().requires_grad_(True) for t in fr["t_articulation"])
            te, code = fr["t_embed"].to(DEV).clone().requires_grad_(True), fr["code_skin"].to(DEV).clone().requires_grad_(True)
            out, _ = warping.skin_logits(P, x, art, te, code, M, spf, mlp.PREC_BF16)
            leaves = [x, art[0], art[1], te, code]
        gs = torch.autograd.grad((out * w).sum(), leaves + [P[k] for k in keys])
        return out.detach(), gs

    o1, g1 = run(True)
    o0, g0 = run(False)
    assert torch.equal(o1, o0)  # inference-mode and training-mode forward: the same arithmetic
    names = (["x", "code"] if net_name == "vis" else ["x", "art_r", "art_d", "t_embed", "code"]) + keys
    for a, b, n in zip(g1, g0, names):
        e = float((a - b).norm() / (b.norm() + 1e-30))
        assert e < 2e-2 and cosine(a, b.cpu()) > 0.999, (n, e)


@pytest.mark.parametrize("prec", [0, 1])
def test_a_tap_belongs_to_the_call_it_was_passed_to(prec):
    """run_chain(tap=d) / eikonal_sdf(tap=...) that fail before their launch (a Python KeyError on a missing weight name -- nothing happens on
    the device) leave nothing behind: d stays empty, and later calls of other nets compute what they compute in a fresh state.
    The tap is an argument of MlpChain.apply / EikonalSdf.apply.  When it travelled through a module global that run_chain armed on its first
    line, the failed call left the global armed until the next run_chain overwrote it; a chain in between that does not come through run_chain
    -- the delta-skin field, warping.skin_logits -- took the stranger's dict for its own, filled it and gave up its fused backward.  The
    `d == {}` directly after skin_logits is the assertion that form fails; the NET_VIS and eikonal steps hold in both forms (run_chain re-arms
    on entry, and eikonal_sdf looks its weights up before it hands the tap on) and pin that the values do not move."""
    from lab4d_amd import mlp, warping
    M, N, D = 2, 4, 64
    spf = N * D
    P, fr, xyz, g = setup(31, M, N, D)
    Pl = {k: (v.to(DEV).clone().requires_grad_(True) if v.dtype.is_floating_point else v.to(DEV)) for k, v in P.items()}
    code_vis, code_base = fr["code_vis"].to(DEV), fr["code_base"].to(DEV)
    x = xyz.reshape(-1, 3).to(DEV)
    w = torch.rand(M * spf, 1, generator=g).to(DEV)
    keys = GRAD_KEYS["vis"]

    def vis():
        xg = x.clone().requires_grad_(True)
        out = mlp.run_chain(mlp.NET_VIS, prec, Pl, xg, spf, conds={0: code_vis})
        return [out.detach()] + list(torch.autograd.grad((out * w).sum(), [xg] + [Pl[k] for k in keys]))

    fresh = vis()
    d = {}
    with pytest.raises(KeyError):
        mlp.run_chain(mlp.NET_FG_BASE, prec, {k: v for k, v in Pl.items() if k != "sdf.weight"}, x, spf, conds={0: code_base, 4: code_base}, tap=d)
    assert d == {}
    # the next chain that does not come through run_chain, directly after the failed call
    art = tuple(t.to(DEV) for t in fr["t_articulation"])
    warping.skin_logits(Pl, x, art, fr["t_embed"].to(DEV), fr["code_skin"].to(DEV), M, spf, prec)
    assert d == {}
    after = vis()
    assert torch.equal(after[0], fresh[0]) and torch.equal(after[1], fresh[1])  # output, point gradient
    for k, a, b in zip(keys, after[2:], fresh[2:]):  # the weight-gradient kernels add their block partials atomically: equal up to the order of those additions
        assert rel_err(a, b.cpu()) < 1e-5, (k, rel_err(a, b.cpu()))
    assert d == {}

    # the eikonal term on the first two rays (blocks 0, 1 of the field pass); the failed call is handed the pattern of blocks 5, 6
    tapped = {}
    mlp.run_chain(mlp.NET_FG_BASE, prec, Pl, x, spf, conds={0: code_base, 4: code_base}, tap=tapped)
    assert tapped.get("emb") is not None
    xe, ray_code = x[:2 * D], code_base[[0, 0]]
    e_fresh = mlp.eikonal_sdf(Pl, xe, ray_code, D, prec)
    with pytest.raises(KeyError):
        mlp.eikonal_sdf(Pl, xe, ray_code, D, prec, prefix="nope.", tap=(tapped, torch.tensor([5, 6], device=DEV)))
    assert torch.equal(mlp.eikonal_sdf(Pl, xe, ray_code, D, prec, tap=None), e_fresh)
