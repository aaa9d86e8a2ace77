"""The skinning kernels (csrc/skinning.hip) entry point by entry point through the C ABI, against float64 references built from the oracle's
own pieces (tests/skinning_cases.py), on every dispatch branch: frame-uniform and per-sample frames, the fused and the two unfused blend
adjoints with and without accumulation, the three routes to the bone parameter gradients, the general and the register-blocked per-frame
Gram kernels at their tile and chunk edges, unaligned rows, NULL in every optional pointer slot, the grid-stride second passes, S = 0 and
the host-side refusals.

For every output and gradient tensor: e_dev = ||device - truth64|| / ||truth64|| <= max(1e-4, 2 e_ref), e_ref being the float32 reference's
distance from the same truth (tests/test_skinning_cases_cpu.py holds e_ref <= 5e-5, so the bound is 1e-4); element-wise
|device - truth64| <= 1e-5 max|truth64| + 1e-4 |truth64|; exactly zero where the truth is zero; and for the per-frame tensors (M,B,.) the
relative-L2 bound on every frame row by itself.  Outputs are pre-filled with -7 (a tensor the kernel writes must be written everywhere);
accumulated outputs start from a random non-zero prefill of the truth's scale and must come back as prefill + truth."""
import pytest
import torch

import skinning_cases as SC
from parity_report import report

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = -7.0


def _lib():
    from lab4d_amd import _lib as L
    return L


def call(name, *a):
    _lib().call(name, *a)
    torch.cuda.synchronize()


def full(*shape):
    return torch.full(shape, FILL, device=DEV)


def on_dev(inp):
    return {k: (v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


def prefill_like(truth, seed):
    """A non-zero float32 prefill of the truth's own scale (CPU)."""
    p = torch.randn(truth.shape, generator=SC.gen(seed)) * max(float(truth.abs().max()), 1e-30)
    return torch.where(p == 0, torch.ones_like(p), p)


def held(tag, dev, truth, ref32, prefill=None, rows=None, what=""):
    """Report e_dev, e_ref and their ratio per tensor, then assert the bounds of the module docstring.  prefill: name -> what an accumulated
    output started from (truth and reference become prefill + themselves).  rows: a slice of the leading dimension to hold by itself."""
    measured, bad = {}, {}
    for k, d in dev.items():
        t, r = truth[k], ref32[k]
        if prefill and k in prefill:
            t, r = t + prefill[k].to(t.device).double(), r + prefill[k].to(r.device)
        d = d.reshape(t.shape)
        if rows is not None:
            d, t, r = d[rows], t[rows], r[rows]
        ok, fig = SC.verdict(d, t, r, per_frame=k in SC.PER_FRAME)
        measured[k + ".e_dev"], measured[k + ".e_ref"] = fig["e_dev"], fig["e_ref"]
        measured[k + ".ratio"] = fig["e_dev"] / fig["e_ref"] if fig["e_ref"] > 0 else 0.0
        if not ok:
            bad[k] = fig
    report("skin_" + tag, measured)
    assert not bad, "%s%s: %s" % (tag, what, bad)


def ids(c):
    return c.name


# ---------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------


def blend_forward(case, D, ent=True, dskin=True):
    S, M, B = case.S, case.M, case.B
    o = {"out": full(S, 3), "ent": full(S) if ent else None, "dskin": full(S) if dskin else None}
    work = full(M * B * 12)
    assert work.data_ptr() % 16 == 0
    call("skin_blend_forward", D["xyz"], D["art_r"], D["art_d"], D["gauss"], D["raw"], D["se3_r"], D["se3_d"], S, case.spf, M, B,
         o["out"], o["ent"], o["dskin"], work)
    o["aff"] = work
    return {k: v for k, v in o.items() if v is not None}


def blend_backward(case, D, truth, params=True, se3=True, accumulate=0, g_ent=True, g_dskin=True, zero_prefill=False, g_raw=None, raw=None):
    """One launch of the blend adjoint.  Returns (device outputs, prefills).  g_raw / raw: caller-supplied (unaligned) tensors."""
    S, M, B, spf = case.S, case.M, case.B, case.spf
    n = int(_lib().lib().lab4d_skin_blend_backward_workspace_floats(S, spf, M, B, 1 if se3 else 0))
    assert n >= M * B * 34 + (0 if (spf % 256 == 0 and se3) else S * (2 * B + 18))
    work = full(n)
    assert work.data_ptr() % 16 == 0
    pre, o = {}, {}

    def start(k, shape, accumulated, seed):
        if accumulated:
            pre[k] = torch.zeros(truth[k].shape) if zero_prefill else prefill_like(truth[k], seed)
            return pre[k].to(DEV).reshape(shape).contiguous()
        return full(*shape)

    o["g_xyz"] = start("g_xyz", (S, 3), accumulate, 11)
    if g_raw is None:
        o["g_raw"] = start("g_raw", (S, B), accumulate, 12)
    else:
        o["g_raw"] = g_raw
        if accumulate:
            pre["g_raw"] = g_raw.detach().cpu().clone()
    if se3:
        o["g_se3"] = start("g_se3", (M, B, 8), True, 13)
    if params:
        o["g_art_r"], o["g_art_d"] = full(M, B, 4), full(M, B, 4)
        o["g_gauss"] = start("g_gauss", (B, 3), True, 14)
    args = [D["xyz"], D["art_r"], D["art_d"], D["gauss"], D["raw"] if raw is None else raw, D["se3_r"], D["se3_d"], D["w_out"],
            D["w_ent"] if g_ent else None, D["w_dskin"] if g_dskin else None, S, spf, M, B, o["g_xyz"], o["g_raw"], o.get("g_se3"),
            o.get("g_art_r"), o.get("g_art_d"), o.get("g_gauss"), work]
    if accumulate:
        call("skin_blend_backward_acc", *args, 1)
    else:
        call("skin_blend_backward", *args)
    return o, pre


def xh_of(D):
    return torch.cat([D["xyz"], torch.ones_like(D["xyz"][:, :1])], -1).contiguous()


# ---------------------------------------------------------------------------------------------------
# bone coordinates
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", SC.BLEND_CASES, ids=ids)
def test_bone_coords_float64_parity(case):
    S, M, B, spf = case.S, case.M, case.B, case.spf
    truth, ref32 = SC.bone_reference(case)
    D = on_dev(SC.blend_inputs(case))
    tab = (D["xyz"], D["art_r"], D["art_d"], D["gauss"])
    out = full(S, 3 * B)
    call("bone_coords_forward", *tab, S, spf, M, B, out)
    aff = full(M, B, 3, 4)
    call("bone_affine", D["art_r"], D["art_d"], D["gauss"], M, B, aff)
    held("bone_fwd_" + case.name, {"xyz_bone": out, "aff": aff}, truth, ref32)
    # the point gradient alone
    gx = full(S, 3)
    call("bone_coords_backward", *tab, D["w_bone"], S, spf, M, B, gx, None, None, None)
    held("bone_bwd_x_" + case.name, {"g_xyz": gx}, truth, ref32)
    # route 1: the three parameter gradients through k_bone_bwd_p, accumulated onto a non-zero prefill; no point gradient
    pre = {k: prefill_like(truth[k], 20 + i) for i, k in enumerate(("g_art_r", "g_art_d", "g_gauss"))}
    o = {k: v.to(DEV) for k, v in pre.items()}
    call("bone_coords_backward", *tab, D["w_bone"], S, spf, M, B, None, o["g_art_r"], o["g_art_d"], o["g_gauss"])
    held("bone_bwd_p_" + case.name, o, truth, ref32, prefill=pre)
    # route 2: bone_coords_backward, then gram_per_frame(g_bone, [x,1]) onto a zeroed G, then bone_params_from_gram
    gx, G = full(S, 3), torch.zeros(M, 3 * B, 4, device=DEV)
    call("bone_coords_backward", *tab, D["w_bone"], S, spf, M, B, gx, None, None, None)
    call("gram_per_frame", D["w_bone"], 3 * B, xh_of(D), 4, S, spf, M, G)
    pre = {"g_gauss": prefill_like(truth["g_gauss"], 23)}
    o = {"g_art_r": full(M, B, 4), "g_art_d": full(M, B, 4), "g_gauss": pre["g_gauss"].to(DEV)}
    call("bone_params_from_gram", D["art_r"], D["art_d"], D["gauss"], G, M, B, o["g_art_r"], o["g_art_d"], o["g_gauss"])
    held("bone_gram_pf_" + case.name, dict(o, g_xyz=gx, G=G), truth, ref32, prefill=pre)
    # route 3 (frame-uniform only): the fused point gradient + Gram matrix (G is zero-filled by the entry), then bone_params_from_gram
    if spf % 256 == 0:
        gx, G = full(S, 3), full(M, 3 * B, 4)
        call("bone_coords_backward_gram", D["xyz"], D["art_r"], D["gauss"], D["w_bone"], S, spf, M, B, gx, G)
        o = {"g_art_r": full(M, B, 4), "g_art_d": full(M, B, 4), "g_gauss": pre["g_gauss"].to(DEV)}
        call("bone_params_from_gram", D["art_r"], D["art_d"], D["gauss"], G, M, B, o["g_art_r"], o["g_art_d"], o["g_gauss"])
        held("bone_gram_fused_" + case.name, dict(o, g_xyz=gx, G=G), truth, ref32, prefill=pre)


def test_bone_params_from_gram_with_every_subset_of_its_outputs_null():
    case = SC.NULL_CASES[0]
    M, B = case.M, case.B
    truth, _ = SC.bone_reference(case)
    D = on_dev(SC.blend_inputs(case))
    G = truth["G"].float().to(DEV).contiguous()
    names = ("g_art_r", "g_art_d", "g_gauss")

    def run(keep):
        o = {"g_art_r": full(M, B, 4), "g_art_d": full(M, B, 4), "g_gauss": torch.full((B, 3), 0.5, device=DEV)}
        call("bone_params_from_gram", D["art_r"], D["art_d"], D["gauss"], G, M, B, *[o[k] if k in keep else None for k in names])
        return {k: o[k] for k in keep}

    whole = run(names)
    assert all(bool((v != FILL).all()) for v in whole.values())
    for n in range(8):
        keep = tuple(k for i, k in enumerate(names) if n >> i & 1)
        part = run(keep)
        for k in keep:  # g_gauss: M atomics per word in any order -- equal to rounding, the written ones bit for bit
            if k == "g_gauss":
                torch.testing.assert_close(part[k], whole[k], rtol=1e-5, atol=1e-6 * float(whole[k].abs().max()))
            else:
                assert torch.equal(part[k], whole[k]), (keep, k)


# ---------------------------------------------------------------------------------------------------
# blend
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", SC.BLEND_CASES, ids=ids)
def test_blend_forward_float64_parity(case):
    truth, ref32, _, _ = SC.blend_reference(case)
    bt, br = SC.bone_reference(case)
    o = blend_forward(case, on_dev(SC.blend_inputs(case)))
    held("blend_fwd_" + case.name, o, dict(truth, aff=bt["aff"]), dict(ref32, aff=br["aff"]))


@pytest.mark.parametrize("params,se3", SC.ADJOINT_WAYS, ids=lambda v: "y" if v else "n")
@pytest.mark.parametrize("case", SC.BLEND_CASES, ids=ids)
def test_blend_adjoint_float64_parity(case, params, se3):
    truth, ref32, _, _ = SC.blend_reference(case)
    o, pre = blend_backward(case, on_dev(SC.blend_inputs(case)), truth, params=params, se3=se3)
    assert set(o) == {"g_xyz", "g_raw"} | ({"g_se3"} if se3 else set()) | ({"g_art_r", "g_art_d", "g_gauss"} if params else set())
    held("blend_bwd_%s_p%d_s%d" % (case.name, params, se3), o, truth, ref32, prefill=pre)


@pytest.mark.parametrize("case,se3", SC.ACC_CASES, ids=lambda v: v.name if isinstance(v, tuple) else ("se3" if v else "nose3"))
def test_blend_adjoint_accumulates_onto_what_the_buffers_hold(case, se3):
    truth, ref32, _, _ = SC.blend_reference(case)
    o, pre = blend_backward(case, on_dev(SC.blend_inputs(case)), truth, params=True, se3=se3, accumulate=1)
    assert {"g_xyz", "g_raw", "g_gauss"} <= set(pre) and all(float(p.abs().min()) > 0 for p in pre.values())
    held("blend_acc_%s_s%d" % (case.name, se3), o, truth, ref32, prefill=pre)


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("case", SC.NULL_CASES, ids=ids)
def test_blend_null_cotangent_equals_zero_cotangent_and_null_outputs_leave_the_others_alone(case):
    """No parameter gradients and no g_se3 here: every output of these launches is written by one thread, so bit equality is meaningful."""
    truth, _, _, _ = SC.blend_reference(case)
    D = on_dev(SC.blend_inputs(case))
    for names in [("w_ent",), ("w_dskin",), ("w_ent", "w_dskin")]:
        Z = dict(D, **{k: torch.zeros_like(D[k]) for k in names})
        zero, _ = blend_backward(case, Z, truth, params=False, se3=False)
        null, _ = blend_backward(case, D, truth, params=False, se3=False, g_ent="w_ent" not in names, g_dskin="w_dskin" not in names)
        _same(zero, null, "NULL %s" % (names,))
        assert all(bool((v != FILL).all()) for v in null.values())
    whole = blend_forward(case, D)
    for ent, dskin in [(False, True), (True, False), (False, False)]:
        part = blend_forward(case, D, ent=ent, dskin=dskin)
        _same(part, {k: v for k, v in whole.items() if k in part}, "forward ent=%s dskin=%s" % (ent, dskin))
        assert set(part) == {"out", "aff"} | ({"ent"} if ent else set()) | ({"dskin"} if dskin else set())


def offset_view(t):
    """A contiguous copy of t that starts 4 bytes into a larger 16-byte-aligned buffer."""
    buf = torch.full((t.numel() + 4,), FILL, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v, buf


@pytest.mark.parametrize("case", SC.UNALIGNED_CASES, ids=ids)
def test_rows_that_start_four_bytes_off_alignment(case):
    """raw, g_raw, g_bone and xyz_bone as views 4 bytes into a larger buffer: the scalar branch of RowTile, including the accumulating store;
    the floats around the views keep their fill."""
    S, M, B, spf = case.S, case.M, case.B, case.spf
    truth, ref32, _, _ = SC.blend_reference(case)
    bt, br = SC.bone_reference(case)
    D = on_dev(SC.blend_inputs(case))
    raw, _ = offset_view(D["raw"])
    for acc in (0, 1):
        start = prefill_like(truth["g_raw"], 31).to(DEV) if acc else full(S, B)
        g_raw, buf = offset_view(start)
        o, pre = blend_backward(case, D, truth, params=True, se3=True, accumulate=acc, g_raw=g_raw, raw=raw)
        held("unaligned_blend_%s_acc%d" % (case.name, acc), o, truth, ref32, prefill=pre)
        assert float(buf[0]) == FILL and bool((buf[1 + S * B:] == FILL).all())
    out = blend_forward(case, dict(D, raw=raw))
    held("unaligned_fwd_" + case.name, {k: out[k] for k in ("out", "ent", "dskin")}, truth, ref32)
    tab = (D["xyz"], D["art_r"], D["art_d"], D["gauss"])
    xb, buf = offset_view(full(S, 3 * B))
    call("bone_coords_forward", *tab, S, spf, M, B, xb)
    assert float(buf[0]) == FILL and bool((buf[1 + S * 3 * B:] == FILL).all())
    gb, _ = offset_view(D["w_bone"])
    gx = full(S, 3)
    call("bone_coords_backward", *tab, gb, S, spf, M, B, gx, None, None, None)
    dev = {"xyz_bone": xb, "g_xyz": gx}
    if spf % 256 == 0:
        gx2, G = full(S, 3), full(M, 3 * B, 4)
        call("bone_coords_backward_gram", D["xyz"], D["art_r"], D["gauss"], gb, S, spf, M, B, gx2, G)
        assert torch.equal(gx2, gx)
        dev["G"] = G
    held("unaligned_bone_" + case.name, dev, bt, br)


# ---------------------------------------------------------------------------------------------------
# gram_per_frame
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("CA,CB", SC.GRAM_PAIRS)
def test_gram_per_frame_float64_parity(CA, CB):
    for spf in SC.GRAM_SPF:
        inp = SC.gram_inputs(CA, CB, spf)
        truth, ref32 = SC.gram_reference(CA, CB, spf)
        S = SC.gram_S(spf)
        out = inp["prefill"].to(DEV).contiguous()
        call("gram_per_frame", inp["A"].to(DEV), CA, inp["Bm"].to(DEV), CB, S, spf, SC.GRAM_M, out)
        ok, fig = SC.verdict(out, truth, ref32, per_frame=True)
        report("skin_gram_%dx%d_spf%d" % (CA, CB, spf), {"out.e_dev": fig["e_dev"], "out.e_ref": fig["e_ref"],
                                                       "out.ratio": fig["e_dev"] / fig["e_ref"] if fig["e_ref"] > 0 else 0.0})
        assert ok, (CA, CB, spf, fig)


# ---------------------------------------------------------------------------------------------------
# gaussian-bone density
# ---------------------------------------------------------------------------------------------------


def gauss_run(D, S, B, truth, best=True, g_xyz=True, g_ibeta=True, zero_prefill=False):
    out, bi = full(S), torch.full((S,), -7, dtype=torch.int32, device=DEV)
    call("gauss_density_forward", D["xyz"], D["centres"], B, D["ibeta"], S, out, bi if best else None)
    if not best:
        return {"out": out}, {}
    pre = {k: (torch.zeros(truth[k].shape) if zero_prefill else prefill_like(truth[k], 40 + i)) for i, k in enumerate(("g_centres", "g_ibeta"))}
    o = {"out": out, "g_xyz": full(S, 3) if g_xyz else None, "g_centres": pre["g_centres"].to(DEV), "g_ibeta": pre["g_ibeta"].to(DEV) if g_ibeta else None}
    call("gauss_density_backward", D["xyz"], D["centres"], B, D["ibeta"], bi, D["w"], S, o["g_xyz"], o["g_centres"], o["g_ibeta"])
    o = {k: v for k, v in o.items() if v is not None}
    o["best"] = bi
    return o, pre


@pytest.mark.parametrize("S,B", SC.GAUSS_CASES)
def test_gauss_density_float64_parity_and_optional_pointers(S, B):
    truth, ref32 = SC.gauss_reference(S, B)
    inp = SC.gauss_inputs(S, B)
    D = on_dev(inp)
    o, pre = gauss_run(D, S, B, truth)
    best = o.pop("best")
    assert torch.equal(best.cpu().long(), SC._centre_dist(inp["xyz"], inp["centres"]).argmin(-1))
    held("gauss_s%d_b%d" % (S, B), o, truth, ref32, prefill=pre)
    nb, _ = gauss_run(D, S, B, truth, best=False)
    assert torch.equal(nb["out"], o["out"])
    for kw, gone in [({"g_xyz": False}, "g_xyz"), ({"g_ibeta": False}, "g_ibeta")]:
        part, pre2 = gauss_run(D, S, B, truth, **kw)
        part.pop("best")
        assert gone not in part
        held("gauss_s%d_b%d_no_%s" % (S, B, gone), part, truth, ref32, prefill=pre2)
        if "g_xyz" in part:
            assert torch.equal(part["g_xyz"], o["g_xyz"])


# ---------------------------------------------------------------------------------------------------
# grid-stride second passes: periodic inputs, the period's truth tiled on the device
# ---------------------------------------------------------------------------------------------------


def _tiled(case):
    """Device inputs of the full case and (truth, ref32) of blend and bone coordinates, tiled on the device; g_gauss is periods x the period's."""
    pc = SC.period_case(case)
    reps = case.M // SC.PERIOD
    P = on_dev(SC.blend_inputs(pc))
    D = {k: v.repeat(reps, *([1] * (v.dim() - 1))) for k, v in P.items() if k not in ("gauss", "frame")}
    D["gauss"] = P["gauss"]
    t, r, _, _ = SC.blend_reference(pc)
    bt, br = SC.bone_reference(pc)

    def tile(ref):
        return {k: (v.to(DEV) * reps if k == "g_gauss" else v.to(DEV).repeat(reps, *([1] * (v.dim() - 1)))) for k, v in ref.items()}

    return D, reps, (tile(t), tile(r)), (tile(bt), tile(br))


def _held_beyond(tag, dev, truth, ref32, first, spf):
    """The whole tensors, then the samples and the frames that only the second pass of the grid-stride loop reaches, by themselves."""
    held(tag, dev, truth, ref32)
    frames = {k: v for k, v in dev.items() if k in SC.PER_FRAME}
    samples = {k: v for k, v in dev.items() if k not in SC.PER_FRAME and k != "g_gauss"}
    held(tag + "_beyond_samples", samples, truth, ref32, rows=slice(first, None), what=" beyond the first %d samples" % first)
    if frames:
        held(tag + "_beyond_frames", frames, truth, ref32, rows=slice(-(-first // spf), None), what=" beyond the first pass's frames")


def test_grid_stride_fused_adjoint_and_fused_bone_gram():
    """S = 524,800 > 2048 blocks x 256: k_blend_bwd<25,true,true> and k_bone_bwd_x<25,true,true> walk a second tile per block."""
    case = SC.GRID_FUSED
    S, M, B, spf = case.S, case.M, case.B, case.spf
    D, reps, (t, r), (bt, br) = _tiled(case)
    first = SC.CAPS["fused"] * 256
    assert S > first
    o, _ = blend_backward(case, D, t, params=True, se3=True, zero_prefill=True)
    _held_beyond("grid_fused_blend_bwd", o, t, r, first, spf)
    gx, G = full(S, 3), full(M, 3 * B, 4)
    call("bone_coords_backward_gram", D["xyz"], D["art_r"], D["gauss"], D["w_bone"], S, spf, M, B, gx, G)
    o = {"g_art_r": full(M, B, 4), "g_art_d": full(M, B, 4), "g_gauss": torch.zeros(B, 3, device=DEV)}
    call("bone_params_from_gram", D["art_r"], D["art_d"], D["gauss"], G, M, B, o["g_art_r"], o["g_art_d"], o["g_gauss"])
    _held_beyond("grid_fused_bone_gram", dict(o, g_xyz=gx, G=G), bt, br, first, spf)


def test_grid_stride_unfused_adjoint_blend_forward_and_bone_coords():
    """S = 2,100,000 > 8192 blocks x 256, spf = 100: k_blend_bwd<18,false,false>, k_blend_fwd, k_bone_fwd and k_bone_bwd_x on their second pass."""
    case = SC.GRID_UNFUSED
    S, M, B, spf = case.S, case.M, case.B, case.spf
    D, reps, (t, r), (bt, br) = _tiled(case)
    first = SC.CAPS["wide"] * 256
    assert S > first
    o = blend_forward(case, D)
    _held_beyond("grid_unfused_blend_fwd", o, dict(t, aff=bt["aff"]), dict(r, aff=br["aff"]), first, spf)
    del o
    o, _ = blend_backward(case, D, t, params=True, se3=True, zero_prefill=True)
    _held_beyond("grid_unfused_blend_bwd", o, t, r, first, spf)
    del o
    tab = (D["xyz"], D["art_r"], D["art_d"], D["gauss"])
    out = full(S, 3 * B)
    call("bone_coords_forward", *tab, S, spf, M, B, out)
    _held_beyond("grid_unfused_bone_fwd", {"xyz_bone": out}, bt, br, first, spf)
    del out
    o = {"g_xyz": full(S, 3), "g_art_r": torch.zeros(M, B, 4, device=DEV), "g_art_d": torch.zeros(M, B, 4, device=DEV),
         "g_gauss": torch.zeros(B, 3, device=DEV)}
    call("bone_coords_backward", *tab, D["w_bone"], S, spf, M, B, o["g_xyz"], o["g_art_r"], o["g_art_d"], o["g_gauss"])
    _held_beyond("grid_unfused_bone_bwd", o, bt, br, first, spf)


def test_grid_stride_gauss_density():
    """S = 2,100,000: the forward's cap of 8192 blocks and the backward's of 1024."""
    S, B, per = SC.GRID_GAUSS
    reps = S // per
    P = on_dev(SC.gauss_inputs(per, B))
    D = dict(P, xyz=P["xyz"].repeat(reps, 1), w=P["w"].repeat(reps))
    t, r = SC.gauss_reference(per, B)
    tile = lambda ref: {k: (v.to(DEV).repeat(reps, *([1] * (v.dim() - 1))) if k in ("out", "g_xyz") else v.to(DEV) * reps) for k, v in ref.items()}
    t, r = tile(t), tile(r)
    o, _ = gauss_run(D, S, B, t, zero_prefill=True)
    o.pop("best")
    held("grid_gauss", o, t, r)
    held("grid_gauss_beyond_fwd", {"out": o["out"]}, t, r, rows=slice(SC.CAPS["wide"] * 256, None))
    held("grid_gauss_beyond_bwd", {"g_xyz": o["g_xyz"]}, t, r, rows=slice(SC.CAPS["gauss_bwd"] * 256, None))


# ---------------------------------------------------------------------------------------------------
# S = 0 and the refusals: decided on the host
# ---------------------------------------------------------------------------------------------------


def _entries(case, D, B=None, spf=None, S=None, M=None):
    """name -> (arguments, positions of the required pointers, prefilled outputs), every buffer sized for the case itself."""
    B0, S0, M0 = case.B, case.S, case.M
    B, spf, S, M = (case.B if B is None else B), (case.spf if spf is None else spf), (case.S if S is None else S), (case.M if M is None else M)
    n = M0 * B0 * 34 + S0 * (2 * B0 + 18)
    o = {k: full(*s) for k, s in {"xyz_bone": (S0, 3 * B0), "g_xyz": (S0, 3), "g_art_r": (M0, B0, 4), "g_art_d": (M0, B0, 4), "g_gauss": (B0, 3),
                                  "G": (M0, 3 * B0, 4), "out": (S0, 3), "ent": (S0,), "dskin": (S0,), "g_raw": (S0, B0), "g_se3": (M0, B0, 8),
                                  "aff": (M0, B0, 12), "work": (n,), "dens": (S0,), "g_centres": (B0, 3), "g_ibeta": (1,),
                                  "gram": (M0, 3 * B0, 4)}.items()}
    o["best"] = torch.full((S0,), -7, dtype=torch.int32, device=DEV)
    tab = [D["xyz"], D["art_r"], D["art_d"], D["gauss"]]
    blend = tab + [D["raw"], D["se3_r"], D["se3_d"]]
    centres, ibeta, bi = D["gauss"], D["gauss"][0, :1].contiguous(), torch.zeros(S0, dtype=torch.int32, device=DEV)
    bwd = blend + [D["w_out"], D["w_ent"], D["w_dskin"], S, spf, M, B, o["g_xyz"], o["g_raw"], o["g_se3"], o["g_art_r"], o["g_art_d"], o["g_gauss"], o["work"]]
    E = {
        "bone_coords_forward": (tab + [S, spf, M, B, o["xyz_bone"]], (0, 1, 2, 3, 8)),
        "bone_coords_backward": (tab + [D["w_bone"], S, spf, M, B, o["g_xyz"], o["g_art_r"], o["g_art_d"], o["g_gauss"]], (0, 1, 2, 3, 4)),
        "bone_coords_backward_gram": ([D["xyz"], D["art_r"], D["gauss"], D["w_bone"], S, spf, M, B, o["g_xyz"], o["G"]], (0, 1, 2, 3, 8, 9)),
        "bone_params_from_gram": ([D["art_r"], D["art_d"], D["gauss"], torch.ones(M0, 3 * B0, 4, device=DEV), M, B, o["g_art_r"], o["g_art_d"], o["g_gauss"]], (0, 1, 2, 3)),
        "bone_affine": ([D["art_r"], D["art_d"], D["gauss"], M, B, o["aff"]], (0, 1, 2, 5)),
        "skin_blend_forward": (blend + [S, spf, M, B, o["out"], o["ent"], o["dskin"], o["work"]], (0, 1, 2, 3, 4, 5, 6, 11, 14)),
        "skin_blend_backward": (bwd, (0, 1, 2, 3, 4, 5, 6, 7, 14, 15, 20)),
        "skin_blend_backward_acc": (bwd + [1], (0, 1, 2, 3, 4, 5, 6, 7, 14, 15, 20)),
        "gauss_density_forward": ([D["xyz"], centres, B, ibeta, S, o["dens"], o["best"]], (0, 1, 3, 5)),
        "gauss_density_backward": ([D["xyz"], centres, B, ibeta, bi, D["w_ent"], S, o["g_xyz"], o["g_centres"], o["g_ibeta"]], (0, 1, 3, 4, 5, 8)),
        "gram_per_frame": ([D["w_bone"], 3 * B, xh_of(D), 4, S, spf, M, o["gram"]], (0, 2, 7)),
    }
    return E, o


def _untouched(o, but=()):
    torch.cuda.synchronize()
    return [k for k, v in o.items() if k not in but and not bool((v == (-7 if v.dtype == torch.int32 else FILL)).all())]


def test_no_samples_is_ok_and_leaves_every_output_alone():
    case = SC.NULL_CASES[1]
    D = on_dev(SC.blend_inputs(case))
    E, o = _entries(case, D, S=0)
    for name, (args, _) in E.items():
        if name in ("bone_params_from_gram", "bone_affine"):
            continue
        call(name, *args)
        if name == "bone_coords_backward_gram":  # its header: G is zero-filled and accumulated
            assert bool((o["G"] == 0).all())
            o["G"].fill_(FILL)
        assert _untouched(o) == [], name
    E, o = _entries(case, D, M=0)
    for name in ("bone_params_from_gram", "bone_affine"):
        call(name, *E[name][0])
        assert _untouched(o) == [], name


def test_refusals_are_decided_on_the_host_before_any_launch():
    L = _lib()
    case = SC.NULL_CASES[1]          # spf = 256: bone_coords_backward_gram is otherwise admissible
    D = on_dev(SC.blend_inputs(case))
    skin = ("bone_coords_forward", "bone_coords_backward", "bone_coords_backward_gram", "skin_blend_forward", "skin_blend_backward", "skin_blend_backward_acc")
    has_spf = skin + ("gram_per_frame",)
    L.PROF = {}
    try:
        def refused(name, args, o, what):
            with pytest.raises(RuntimeError, match=name):
                L.call(name, *args)
            assert _untouched(o) == [], (name, what)

        for name in skin:
            E, o = _entries(case, D, B=24)
            refused(name, E[name][0], o, "B = 24")
        for name in has_spf:
            E, o = _entries(case, D, S=case.M * case.spf + 1)   # (never launched: the buffers hold M*spf samples)
            refused(name, E[name][0], o, "M*spf < S")
            E, o = _entries(case, D, spf=0)
            refused(name, E[name][0], o, "spf = 0")
        E, o = _entries(case, D)
        for name, (args, required) in E.items():
            for i in required:
                refused(name, args[:i] + [None] + args[i + 1:], o, "NULL in slot %d" % i)
        E, o = _entries(case, D, spf=100, S=200)
        refused("bone_coords_backward_gram", E["bone_coords_backward_gram"][0], o, "spf = 100")
        for CA, CB in [(81, 4), (4, 17), (72, 9), (0, 4), (4, 0)]:
            A, Bm = torch.ones(8, max(CA, 1), device=DEV), torch.ones(8, max(CB, 1), device=DEV)
            out = full(1, max(CA, 1), max(CB, 1))
            refused("gram_per_frame", [A, CA, Bm, CB, 8, 8, 1, out], {"out": out}, (CA, CB))
        E, o = _entries(case, D)
        args = list(E["gauss_density_backward"][0])
        args[1], args[2], args[8] = torch.zeros(65, 3, device=DEV), 65, full(65, 3)
        refused("gauss_density_backward", args, dict(o, g_centres=args[8]), "B = 65")
        # one or two of the three parameter gradients: refused before the point gradient is launched
        base = E["bone_coords_backward"][0]
        for keep in [(10,), (11,), (12,), (10, 11), (11, 12), (10, 12)]:
            args = [a if (i < 10 or i in keep) else None for i, a in enumerate(base)]
            refused("bone_coords_backward", args, o, "parameter gradients %s only" % (keep,))
        torch.cuda.synchronize()
        assert L.prof_summary() == {}, "a refused call launched nothing: it has no place in the per-kernel profile"
    finally:
        L.PROF = None
