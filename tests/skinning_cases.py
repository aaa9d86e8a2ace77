"""Cases, inputs and float64 references for the skinning kernels (csrc/skinning.hip), entry point by entry point.

The truth of the blend is built from the oracle's own pieces (oracle/lab4d_oracle.py) with the delta-skin logits `raw` (S,B) as an INPUT, so
that no MLP stands between the kernels and their reference:

    c = O.get_bone_coords(xyz, art) / gauss;  skin = -(|c|^2 + relu(raw) * 0.1);  out = O.dual_quaternion_skinning(se3, xyz, softmax(skin))
    ent = O.cross_entropy_skin_loss(skin);    dskin = mean_b (relu(raw) * 0.1)^2

run on float64 tensors, gradients by autograd; `e_ref` is the same reference run in float32, in the metric the device is held to (relative L2,
compared in float64).  The inputs keep every discontinuity of the operation (the arg-max anchor, the ReLU, the hemisphere sign, the nearest
centre) away from rounding, so NO sample is excluded from any comparison; tests/test_skinning_cases_cpu.py asserts those margins, the
reference's own error and a census of the kernel instantiations the case lists reach.  Everything here runs without a GPU;
tests/test_gpu_skinning_kernels.py runs the device against the same (cached, never modified) references."""
import functools
import itertools
from collections import namedtuple

import torch

from oracle import lab4d_oracle as O
from raypath_cases import E_REF_MAX, bound, gen, rel_l2  # the house metric and bound, shared with the ray path  # noqa: F401

ANCHOR_MARGIN = 1e-3     # top-two gap of skin, every sample
RELU_MARGIN = 1e-2       # |raw|, every entry outside the planted column of exact zeros
ZERO_COLUMN = 3
HEMI_MARGIN = 1e-2       # |q_anchor . q_b|, every (sample, bone)
CENTRE_GAP = 1e-4        # distance to the second-nearest centre minus distance to the nearest, every sample
ATOL, RTOL = 1e-5, 1e-4  # element-wise: |dev - truth| <= ATOL max|truth| + RTOL |truth|
BONES = (25, 18)
PERIOD = 50              # frames per period of the grid-stride inputs

BlendCase = namedtuple("BlendCase", "name M spf S B")


def _case(M, spf, S, B):
    return BlendCase("m%d_spf%d_s%d_b%d" % (M, spf, S, B), M, spf, S, B)


SHAPES = [(1, 1, 1), (2, 63, 126), (3, 100, 257), (1, 256, 255), (1, 256, 1), (2, 256, 512), (3, 256, 700), (2, 512, 1024)]
BLEND_CASES = [_case(M, spf, S, B) for B in BONES for M, spf, S in SHAPES]
ADJOINT_WAYS = list(itertools.product((True, False), (True, False)))   # (parameter gradients asked for, g_se3 given)
# (case, g_se3 given): one non-uniform, one fused and one uniform-unfused adjoint per bone count
ACC_CASES = [(_case(M, spf, S, B), se3) for B in BONES for (M, spf, S), se3 in [((2, 63, 126), True), ((3, 256, 700), True), ((2, 256, 512), False)]]
UNALIGNED_CASES = [_case(3, 100, 257, 25), _case(3, 256, 700, 18)]
NULL_CASES = [_case(2, 63, 126, 18), _case(2, 256, 512, 25)]
GRAM_PAIRS = [(75, 4), (54, 4), (25, 8), (18, 8), (25, 10), (18, 10), (80, 8), (1, 1), (40, 16), (7, 3)]
GRAM_SPF = (1, 127, 128, 129, 1024, 1025)
GRAM_M = 3
GAUSS_CASES = [(1, 25), (257, 18), (1000, 25)]                          # (S, B)
# grid-stride second pass: periodic inputs (PERIOD frames), neither cap x 256 is a multiple of the period's samples
GRID_FUSED = BlendCase("grid_fused", 2050, 256, 2050 * 256, 25)          # 524,800 samples over the cap of 2048 blocks
GRID_UNFUSED = BlendCase("grid_unfused", 21000, 100, 21000 * 100, 18)    # 2,100,000 samples over the cap of 8192 blocks
GRID_GAUSS = (2100000, 25, 5000)                                         # S, B, period in samples: forward cap 8192, backward cap 1024
CAPS = {"fused": 2048, "wide": 8192, "gauss_bwd": 1024}


def gram_S(spf, M=GRAM_M):
    return M * spf - 5 if M * spf > 5 else M * spf - 1


# ---------------------------------------------------------------------------------------------------
# the metric: one verdict for a device tensor, shared by the GPU tests and the CPU "the metric sees it" tests
# ---------------------------------------------------------------------------------------------------


def _rel(d, t):
    n, e = float(t.norm()), float((d - t).norm())
    return e / n if n > 0 else (0.0 if e == 0 else float("inf"))


def verdict(dev, truth, ref32, per_frame=False):
    """(ok, figures) of one device tensor against its float64 truth, compared on the device the truth lives on:
    e_dev = rel_l2 <= max(1e-4, 2 e_ref); element-wise |dev - truth| <= ATOL max|truth| + RTOL |truth|; exactly zero where the truth is zero;
    per_frame: the relative-L2 bound again on every row of the leading (frame) dimension, each against that row's own e_ref."""
    t = truth
    d, r = dev.detach().to(t.device).double(), ref32.to(t.device).double()
    assert d.shape == t.shape == r.shape, (d.shape, t.shape, r.shape)
    fig = {"e_dev": _rel(d, t), "e_ref": _rel(r, t)}
    tmax = float(t.abs().max()) if t.numel() else 0.0
    fig["excess"] = float(((d - t).abs() - (ATOL * tmax + RTOL * t.abs())).max()) if t.numel() else -0.0
    fig["nonzero_at_zero"] = int((d[t == 0] != 0).sum())
    ok = fig["e_dev"] <= bound(fig["e_ref"]) and fig["excess"] <= 0 and fig["nonzero_at_zero"] == 0
    if per_frame and t.numel():
        M = t.shape[0]
        en = (d - t).reshape(M, -1).norm(dim=1)
        rn = (r - t).reshape(M, -1).norm(dim=1)
        tn = t.reshape(M, -1).norm(dim=1)
        live = tn > 0
        row = torch.where(live, en / tn.clamp_min(1e-300), torch.zeros_like(en))
        row_b = torch.where(live, (2.0 * rn / tn.clamp_min(1e-300)).clamp_min(1e-4), torch.full_like(en, 1e-4))
        fig["worst_frame_e_dev"] = float(row.max())
        fig["frames_over"] = int((row > row_b).sum()) + int((en[~live] != 0).sum())
        ok = ok and fig["frames_over"] == 0
    return ok, fig


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------


def _unit(q):
    return q / q.norm(dim=-1, keepdim=True)


def _dual_of(q, t):
    """The dual part of the dual quaternion of rotation q and translation t: 0.5 (0,t) q."""
    return 0.5 * O.quaternion_mul(t, q)


def frame_of(S, spf):
    return torch.arange(S) // spf


def _skin64(inp):
    fr = inp["frame"]
    c = O.get_bone_coords(inp["xyz"].double(), (inp["art_r"].double()[fr], inp["art_d"].double()[fr])) / inp["gauss"].double()
    return -(c.pow(2).sum(-1) + torch.relu(inp["raw"].double()) * 0.1)


@functools.lru_cache(maxsize=None)
def blend_inputs(case):
    """float32 CPU inputs of one case (cached; callers must not modify them): points, bone tables, logits, se3 tables with ~40% of the
    (frame, bone) rows negated (the same transforms: the hemisphere fix has work to do), and the three cotangents (loss weights)."""
    M, spf, S, B = case.M, case.spf, case.S, case.B
    g = gen(7000 + 13 * M + 3 * spf + S + 101 * B)
    inp = {"frame": frame_of(S, spf)}
    centres = 0.06 * torch.randn(B, 3, generator=g)
    inp["art_r"] = _unit(torch.cat([torch.ones(M, B, 1), 0.6 * torch.randn(M, B, 3, generator=g)], -1))
    inp["art_d"] = _dual_of(inp["art_r"], centres[None] + 0.01 * torch.randn(M, B, 3, generator=g))
    inp["gauss"] = 0.06 * torch.exp(0.1 * torch.randn(B, 3, generator=g))
    raw = torch.randn(S, B, generator=g) * 3
    raw = torch.where(raw < 0, raw - RELU_MARGIN, raw + RELU_MARGIN)
    raw[:, ZERO_COLUMN] = 0
    inp["raw"] = raw
    # se3: rotations near the identity (every pairwise |q_a . q_b| is far from 0), then exactly round(0.4 B) rows per frame negated
    for _ in range(20):
        r = _unit(torch.cat([torch.ones(M, B, 1), 0.3 * torch.randn(M, B, 3, generator=g)], -1))
        if float(torch.einsum("mak,mbk->mab", r, r).abs().min()) >= 10 * HEMI_MARGIN:
            break
    d = _dual_of(r, 0.02 * torch.randn(M, B, 3, generator=g))
    flip = torch.ones(M, B, 1)
    for m in range(M):
        flip[m, torch.randperm(B, generator=g)[: round(0.4 * B)]] = -1
    inp["se3_r"], inp["se3_d"] = (r * flip).contiguous(), (d * flip).contiguous()
    inp["xyz"] = 0.08 * torch.randn(S, 3, generator=g)
    for _ in range(100):  # the anchor margin: offending points are redrawn, deterministically, until none is left
        top = _skin64(inp).topk(2, -1)[0]
        bad = (top[:, 0] - top[:, 1]) < 2 * ANCHOR_MARGIN
        if not bool(bad.any()):
            break
        inp["xyz"][bad] = 0.08 * torch.randn(int(bad.sum()), 3, generator=g)
    inp["w_out"] = torch.randn(S, 3, generator=g)
    inp["w_ent"] = torch.randn(S, generator=g)
    inp["w_dskin"] = torch.randn(S, generator=g) * 10
    inp["w_bone"] = torch.randn(S, 3 * B, generator=g)
    return inp


BLEND_LEAVES = ("xyz", "art_r", "art_d", "gauss", "raw", "se3_r", "se3_d")
BONE_LEAVES = ("xyz", "art_r", "art_d", "gauss")
PER_FRAME = ("g_se3", "g_art_r", "g_art_d", "aff", "G")   # (M,B,.) tensors: held per frame row as well


def run_blend(inp, dtype, signs=None):
    """The kernel-level reference: outputs and the gradient of every input under the case's cotangents, detached.  `signs` (S,B) overrides
    the hemisphere signs (only the CPU test's synthetic perturbation uses it)."""
    S = inp["xyz"].shape[0]
    fr = inp["frame"]
    L = {k: inp[k].to(dtype).clone().requires_grad_(True) for k in BLEND_LEAVES}
    c = O.get_bone_coords(L["xyz"], (L["art_r"][fr], L["art_d"][fr])) / L["gauss"]
    delta = torch.relu(L["raw"]) * 0.1
    skin = -(c.pow(2).sum(-1) + delta)
    se3 = (L["se3_r"][fr], L["se3_d"][fr])                                   # one "frame" per sample: (S,B,4)
    if signs is None:
        out = O.dual_quaternion_skinning(se3, L["xyz"][:, None], skin.softmax(-1)[:, None]).reshape(S, 3)
    else:
        p = (skin.softmax(-1) * signs.to(dtype))[..., None]
        qr, qd = (p * se3[0]).sum(1), (p * se3[1]).sum(1)
        inv = qr.norm(dim=-1, keepdim=True).reciprocal()
        out = O.dual_quaternion_apply((qr * inv, qd * inv), L["xyz"])
    ent = O.cross_entropy_skin_loss(skin)
    dskin = delta.pow(2).mean(-1)
    loss = (out * inp["w_out"].to(dtype)).sum() + (ent * inp["w_ent"].to(dtype)).sum() + (dskin * inp["w_dskin"].to(dtype)).sum()
    g = dict(zip(BLEND_LEAVES, torch.autograd.grad(loss, [L[k] for k in BLEND_LEAVES])))
    res = {"out": out, "ent": ent, "dskin": dskin, "g_xyz": g["xyz"], "g_raw": g["raw"], "g_se3": torch.cat([g["se3_r"], g["se3_d"]], -1),
           "g_art_r": g["art_r"], "g_art_d": g["art_d"], "g_gauss": g["gauss"]}
    anchor = skin.argmax(-1)
    qa = torch.gather(se3[0], 1, anchor.view(S, 1, 1).expand(S, 1, 4))
    aux = {"skin": skin, "anchor": anchor, "hemi_dot": (qa * se3[0]).sum(-1)}
    return {k: v.detach() for k, v in res.items()}, {k: v.detach() for k, v in aux.items()}


@functools.lru_cache(maxsize=None)
def blend_reference(case):
    """(truth64, ref32, aux64, aux32).  Cached; callers must not modify it."""
    inp = blend_inputs(case)
    t, at = run_blend(inp, torch.float64)
    r, ar = run_blend(inp, torch.float32)
    return t, r, at, ar


def _coords(xyz, art_r, art_d, gauss, fr):
    return O.get_bone_coords(xyz, (art_r[fr], art_d[fr])) / gauss


def per_frame_gram(A, Bm, spf, M, dtype=torch.float64):
    """out[m] = A[frame m]^T Bm[frame m], one einsum per frame."""
    A, Bm = A.to(dtype), Bm.to(dtype)
    out = torch.zeros(M, A.shape[1], Bm.shape[1], dtype=dtype)
    for m in range(M):
        out[m] = torch.einsum("si,sj->ij", A[m * spf:(m + 1) * spf], Bm[m * spf:(m + 1) * spf])
    return out


def run_bone(inp, dtype, M):
    """Bone coordinates alone: the (S,3B) rows, their adjoint under the (S,3B) cotangent w_bone, the per-frame Gram matrix of that cotangent
    with [x,1], and the affine table read off get_bone_coords at 0, e_x, e_y, e_z."""
    S = inp["xyz"].shape[0]
    fr = inp["frame"]
    L = {k: inp[k].to(dtype).clone().requires_grad_(True) for k in BONE_LEAVES}
    out = _coords(L["xyz"], L["art_r"], L["art_d"], L["gauss"], fr).reshape(S, -1)
    g = dict(zip(BONE_LEAVES, torch.autograd.grad((out * inp["w_bone"].to(dtype)).sum(), [L[k] for k in BONE_LEAVES])))
    with torch.no_grad():
        B = inp["gauss"].shape[0]
        probe = torch.cat([torch.zeros(1, 3, dtype=dtype), torch.eye(3, dtype=dtype)]).repeat(M, 1)          # (4M,3), frame = i // 4
        c = _coords(probe, L["art_r"], L["art_d"], L["gauss"], frame_of(4 * M, 4)).reshape(M, 4, 3 * B)
        aff = torch.cat([(c[:, 1:] - c[:, :1]).transpose(1, 2), c[:, 0, :, None]], -1)                       # (M,3B,4): [linear | offset]
        xh = torch.cat([inp["xyz"].to(dtype), torch.ones(S, 1, dtype=dtype)], -1)
        G = per_frame_gram(inp["w_bone"], xh, int(inp["spf"]), M, dtype)
    res = {"xyz_bone": out, "g_xyz": g["xyz"], "g_art_r": g["art_r"], "g_art_d": g["art_d"], "g_gauss": g["gauss"], "aff": aff, "G": G}
    return {k: v.detach() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def bone_reference(case):
    inp = dict(blend_inputs(case), spf=case.spf)
    return run_bone(inp, torch.float64, case.M), run_bone(inp, torch.float32, case.M)


# ---------------------------------------------------------------------------------------------------
# gram_per_frame
# ---------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def gram_inputs(CA, CB, spf, M=GRAM_M):
    S = gram_S(spf, M)
    g = gen(8000 + 17 * CA + 5 * CB + spf)
    return {"A": torch.randn(S, CA, generator=g), "Bm": torch.randn(S, CB, generator=g), "prefill": torch.randn(M, CA, CB, generator=g) * spf ** 0.5}


@functools.lru_cache(maxsize=None)
def gram_reference(CA, CB, spf, M=GRAM_M):
    """(truth64, ref32) of prefill + the per-frame product: the accumulation onto a non-zero output is part of the operation."""
    inp = gram_inputs(CA, CB, spf, M)
    return (inp["prefill"].double() + per_frame_gram(inp["A"], inp["Bm"], spf, M),
            inp["prefill"] + per_frame_gram(inp["A"], inp["Bm"], spf, M, torch.float32))


# ---------------------------------------------------------------------------------------------------
# gaussian-bone density
# ---------------------------------------------------------------------------------------------------


def _centre_dist(xyz, centres):
    return (xyz.double()[:, None] - centres.double()[None]).norm(dim=-1)


@functools.lru_cache(maxsize=None)
def gauss_inputs(S, B):
    """Points within 0.03 of some centre (exp(-0.5 (0.03/0.01)^2) = 0.011: no underflow anywhere), the nearest centre clear of the second."""
    g = gen(9000 + S + 31 * B)
    centres = 0.06 * torch.randn(B, 3, generator=g)

    def draw(n):
        d = torch.randn(n, 3, generator=g)
        return centres[torch.randint(0, B, (n,), generator=g)] + d / d.norm(dim=-1, keepdim=True) * (0.029 * torch.rand(n, 1, generator=g))

    xyz = draw(S)
    for _ in range(100):
        d2 = _centre_dist(xyz, centres).topk(2, -1, largest=False)[0]
        bad = (d2[:, 1] - d2[:, 0]) < 2 * CENTRE_GAP
        if not bool(bad.any()):
            break
        xyz[bad] = draw(int(bad.sum()))
    return {"xyz": xyz, "centres": centres, "ibeta": torch.tensor([100.0]) + torch.rand(1, generator=g), "w": torch.randn(S, generator=g)}


def run_gauss(inp, dtype):
    """O.gauss_density with the centres and ibeta as leaves: rest bones with the identity rotation and the dual part (0, c/2) have their
    centres at c exactly; logibeta = log(ibeta)."""
    L = {k: inp[k].to(dtype).clone().requires_grad_(True) for k in ("xyz", "centres", "ibeta")}
    B = L["centres"].shape[0]
    rest = (torch.tensor([1.0, 0, 0, 0], dtype=dtype).repeat(1, B, 1), torch.cat([torch.zeros(B, 1, dtype=dtype), L["centres"] / 2], -1)[None])
    out = O.gauss_density({"warp.logibeta": L["ibeta"].log()}, L["xyz"], rest).reshape(-1)
    g = torch.autograd.grad((out * inp["w"].to(dtype)).sum(), [L["xyz"], L["centres"], L["ibeta"]])
    res = {"out": out, "g_xyz": g[0], "g_centres": g[1], "g_ibeta": g[2]}
    return {k: v.detach() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def gauss_reference(S, B):
    inp = gauss_inputs(S, B)
    return run_gauss(inp, torch.float64), run_gauss(inp, torch.float32)


# ---------------------------------------------------------------------------------------------------
# grid-stride cases: one period of frames, tiled by the caller
# ---------------------------------------------------------------------------------------------------


def period_case(case):
    assert case.M % PERIOD == 0 and case.S == case.M * case.spf
    return BlendCase(case.name + "_period", PERIOD, case.spf, PERIOD * case.spf, case.B)


# ---------------------------------------------------------------------------------------------------
# census: which (kernel, template arguments) a call reaches, the way the host code dispatches
# ---------------------------------------------------------------------------------------------------


def reached(entry, B=None, spf=1, g_se3=True, params=True, accumulate=False, CB=None, g_xyz=True):
    uni = "true" if spf % 256 == 0 else "false"
    if entry == "bone_coords_forward":
        return {"k_bone_fwd<%d,%s>" % (B, uni)}
    if entry == "bone_coords_backward":
        return ({"k_bone_bwd_x<%d,%s,false>" % (B, uni)} if g_xyz else set()) | ({"k_bone_bwd_p<%d>" % B} if params else set())
    if entry == "bone_coords_backward_gram":
        assert spf % 256 == 0
        return {"k_bone_bwd_x<%d,true,true>" % B}
    if entry == "bone_params_from_gram":
        return {"k_bone_param_from_gram"}
    if entry == "bone_affine":
        return {"k_bone_affine"}
    if entry == "gram_per_frame":
        return {"k_gram_pf_rb<%d>" % CB if CB in (4, 8, 10) else "k_gram_pf"}
    if entry == "skin_blend_forward":
        return {"k_bone_affine", "k_blend_fwd<%d,%s>" % (B, uni)}
    if entry == "skin_blend_backward":
        fused = spf % 256 == 0 and g_se3
        acc = "true" if accumulate else "false"
        ks = {"k_bone_affine", "k_blend_bwd<%d,%s,%s,%s>" % (B, uni, "true" if fused else "false", acc)}
        if g_se3 and not fused:
            ks |= reached("gram_per_frame", CB=8)
        if params:
            if not fused:
                ks |= reached("gram_per_frame", CB=10)
            ks |= {"k_bone_gram_from_moments", "k_bone_param_from_gram"}
        return ks
    if entry == "gauss_density_forward":
        return {"k_gauss_density_fwd"}
    if entry == "gauss_density_backward":
        return {"k_gauss_density_bwd"}
    raise KeyError(entry)


def every_instantiation():
    ks = {"k_bone_affine", "k_bone_param_from_gram", "k_bone_gram_from_moments", "k_gauss_density_fwd", "k_gauss_density_bwd", "k_gram_pf",
          "k_gram_pf_rb<4>", "k_gram_pf_rb<8>", "k_gram_pf_rb<10>"}
    for B in BONES:
        ks |= {"k_bone_bwd_p<%d>" % B, "k_bone_bwd_x<%d,true,true>" % B}
        for uni in ("true", "false"):
            ks |= {"k_bone_fwd<%d,%s>" % (B, uni), "k_bone_bwd_x<%d,%s,false>" % (B, uni), "k_blend_fwd<%d,%s>" % (B, uni)}
            for acc in ("true", "false"):
                ks.add("k_blend_bwd<%d,%s,false,%s>" % (B, uni, acc))
        for acc in ("true", "false"):
            ks.add("k_blend_bwd<%d,true,true,%s>" % (B, acc))
    return ks
