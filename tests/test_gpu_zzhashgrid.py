"""GPU check of the hash-grid encoding kernels (csrc/hashgrid.hip) through the Python wrapper lab4d_amd/hashgrid.py against
oracle/hashgrid_oracle.py (parity vs the reference is unpinned by nature: the reference has no hash grid).

First hardware run (round 2) found the kernels 2e-5 off at the finest level (res 2048): the compiler had fused
`x * res - floor(x * res)` into fma(x, res, -floor), i.e. an UNROUNDED product, which moves the fractional cell position by up
to ulp(x * res) = 1.2e-4.  The product is now opaque to the optimiser (mul_rn of csrc/hd_math.hpp) and the forward bound
is a few ulp."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("L,F,log2_T,n_min,n_max,S", [(16, 2, 19, 16, 2048, 65573), (8, 4, 10, 4, 128, 1000)])
def test_hash_encode_matches_the_oracle(L, F, log2_T, n_min, n_max, S):
    from lab4d_amd import hashgrid
    from oracle import hashgrid_oracle as HO
    g = torch.Generator().manual_seed(L + F)
    res = hashgrid.level_resolutions(L, n_min, n_max)
    assert res == HO.level_resolutions(L, n_min, n_max)
    x = torch.rand(S, 3, generator=g)
    x[0], x[1] = 0.0, 1.0
    table = torch.randn(L, 1 << log2_T, F, generator=g) * 0.1
    n_ref = min(S, 4096)  # the oracle on a prefix; the tail is covered by linearity below
    xt, tt = x[:n_ref].clone().requires_grad_(True), table.clone().requires_grad_(True)
    ref = HO.hash_encode(xt, tt, res, log2_T)
    c = torch.randn(S, L * F, generator=g)
    gx_ref, gt_ref = torch.autograd.grad((ref * c[:n_ref]).sum(), [xt, tt])
    xd, td = x.to(DEV).requires_grad_(True), table.to(DEV).requires_grad_(True)
    rd = torch.tensor(res, dtype=torch.int32, device=DEV)
    out = hashgrid.hash_encode(xd, td, rd, log2_T)
    e_out = float((out[:n_ref].detach().cpu() - ref.detach()).abs().max())
    assert e_out < 2e-6, "forward: max abs error %.3e" % e_out  # tri-linear blend of 8 entries of magnitude 0.1: a few ulp
    gx, gt = torch.autograd.grad((out[:n_ref] * c[:n_ref].to(DEV)).sum(), [xd, td])
    assert torch.allclose(gt.cpu(), gt_ref, atol=1e-4)
    inside = ((x[:n_ref] > 0) & (x[:n_ref] < 1)).all(-1)
    assert torch.allclose(gx[:n_ref].cpu()[inside], gx_ref[inside], atol=2e-3 * max(1.0, float(gx_ref.abs().max())))
    # size-independent property on the full batch: linear in the table
    t2 = torch.randn_like(table).to(DEV) * 0.1
    a = hashgrid.hash_encode(xd.detach(), td.detach(), rd, log2_T)
    b = hashgrid.hash_encode(xd.detach(), t2, rd, log2_T)
    ab = hashgrid.hash_encode(xd.detach(), td.detach() * 2 - t2 * 0.5, rd, log2_T)
    assert torch.allclose(ab, 2 * a - 0.5 * b, atol=1e-5)


@pytest.mark.parametrize("prec_name,tol,gtol", [("f32", 2e-4, 2e-3), ("bf16", 3e-2, 5e-2), ("bench", 3e-2, 5e-2)])
def test_hash_field_matches_the_oracle(prec_name, tol, gtol):
    """The hash-grid FIELD (hash encoding -> fused geometry / colour chains -> VolSDF density; lab4d_amd/hashfield.py) against its
    torch-CPU restatement: outputs and the gradients of the table, every Linear and the points.  Parity unpinned against the
    reference (it has no hash grid); fp32 chains to 2e-4, bf16 chains to their rounding."""
    from lab4d_amd import hashfield, mlp
    from oracle import hashgrid_oracle as HO
    cfg = {"L": 16, "F": 2, "log2_T": 14, "n_min": 16, "n_max": 512}
    P, cfg = hashfield.make_weights(3, cfg, sdf_bias=0.01)
    P["hash.table"] = P["hash.table"] * 3e3  # features of order 0.3 so that the nets see a signal
    g = torch.Generator().manual_seed(5)
    S = 1000
    xyz = (torch.rand(S, 3, generator=g) * 2 - 1) * 0.15  # the box is +-0.12: about half of the points lie outside it (no density, no colour, no gradient)
    dirs = torch.nn.functional.normalize(torch.randn(S, 3, generator=g), dim=-1)
    names = [k for k in P if k != "aabb"]
    cw = [torch.randn(S, 3, generator=g), torch.randn(S, 1, generator=g)]

    def run(fwd, dev):
        Pl = {k: (v.to(dev).clone().requires_grad_(True) if k in names else v.to(dev)) for k, v in P.items()}
        x = xyz.to(dev).clone().requires_grad_(True)
        rgb, dens = fwd(Pl, x, dirs.to(dev))
        loss = (rgb * cw[0].to(dev)).sum() + (dens * cw[1].to(dev)).sum() * 1e-2
        gs = torch.autograd.grad(loss, [Pl[k] for k in names] + [x])
        return rgb, dens, dict(zip(names + ["xyz"], gs))

    prec = mlp.PREC_F32 if prec_name == "f32" else mlp.PREC_BF16
    rr, rd, rg = run(lambda Pl, x, d: HO.hash_field_forward(Pl, cfg, x, d), "cpu")
    if prec_name == "bench":  # the configuration `bench.py --config hash` times: bf16 chains on the compacted inside-box samples, packed-fp16 table gradient on the hashed levels
        dr, dd, dg = run(lambda Pl, x, d: hashfield.forward_compacted(Pl, cfg, x, d, 1024, prec=prec, table_grad_f16=True)[:2], DEV)
    else:
        dr, dd, dg = run(lambda Pl, x, d: hashfield.forward(Pl, cfg, x, d, spf=S, prec=prec), DEV)
    rel = lambda a, b: float((a.detach().cpu() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-12))
    assert rel(dr, rr) < tol and rel(dd, rd) < tol, (rel(dr, rr), rel(dd, rd))
    # fp32: max-norm; bf16: relative L2 per tensor, like the bf16 bounds of the training-graph tests (a table entry sees a handful of
    # samples, its bf16 rounding noise does not average out entry by entry)
    rl2 = lambda a, b: float((a.detach().cpu() - b.detach()).norm() / b.detach().norm().clamp_min(1e-20))
    for k in names + ["xyz"]:
        e = rel(dg[k], rg[k]) if prec_name == "f32" else rl2(dg[k], rg[k])
        assert e < gtol, (k, e)


@pytest.mark.parametrize("prec_name", ["f32", "bf16"])
def test_compacted_field_equals_the_full_field(prec_name):
    """hashfield.forward_compacted (round 6: the field on the inside-box samples only, device-side stream compaction into a static-capacity buffer)
    against hashfield.forward on every sample: colour / density identical sample by sample (the per-sample arithmetic does not depend on the row),
    zeros outside the box, the gradients of the table, every Linear and the points equal up to the summation order; a capacity below the count is
    reported by the overflow flag."""
    from lab4d_amd import hashfield, mlp
    cfg = {"L": 16, "F": 2, "log2_T": 14, "n_min": 16, "n_max": 512}
    P, cfg = hashfield.make_weights(3, cfg, sdf_bias=0.01)
    P["hash.table"] = P["hash.table"] * 3e3
    g = torch.Generator().manual_seed(7)
    S = 5000
    xyz = (torch.rand(S, 3, generator=g) * 2 - 1) * 0.2  # the box is +-0.12: ~22 % of the points lie inside
    dirs = torch.nn.functional.normalize(torch.randn(S, 3, generator=g), dim=-1)
    names = [k for k in P if k != "aabb"]
    cw = [torch.randn(S, 3, generator=g).to(DEV), torch.randn(S, 1, generator=g).to(DEV)]
    prec = mlp.PREC_F32 if prec_name == "f32" else mlp.PREC_BF16
    n_inside = int(((xyz.abs() <= 0.12).all(-1)).sum())

    def run(compact, cap=None):
        Pl = {k: (v.to(DEV).clone().requires_grad_(True) if k in names else v.to(DEV)) for k, v in P.items()}
        x = xyz.to(DEV).clone().requires_grad_(True)
        if compact:
            rgb, dens, count, ovf = hashfield.forward_compacted(Pl, cfg, x, dirs.to(DEV), cap, prec=prec)
        else:
            (rgb, dens), count, ovf = hashfield.forward(Pl, cfg, x, dirs.to(DEV), spf=S, prec=prec), None, None
        gs = torch.autograd.grad((rgb * cw[0]).sum() + (dens * cw[1]).sum() * 1e-2, [Pl[k] for k in names] + [x])
        return rgb.detach(), dens.detach(), dict(zip(names + ["xyz"], gs)), count, ovf

    r0, d0, g0, _, _ = run(False)
    r1, d1, g1, count, ovf = run(True, cap=2048)
    assert int(count) == n_inside and not bool(ovf) and 500 < n_inside < 2048
    assert torch.equal(r1, r0) and torch.equal(d1, d0)
    out = (xyz.abs() > 0.12).any(-1).to(DEV)
    assert float(r1[out].abs().max()) == 0.0 and float(d1[out].abs().max()) == 0.0
    for k in names + ["xyz"]:
        e = float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-20))
        assert e < (1e-5 if prec_name == "f32" else 2e-3), (k, e)  # (bf16: the weight-gradient kernels split the sample axis differently over fp32 atomics; the operands are the same)
    # too small a buffer: flagged, never silent
    *_, ovf2 = run(True, cap=256)
    assert bool(ovf2)


def test_packed_fp16_table_gradient_matches_the_fp32_accumulation():
    """Round 6: the hashed levels' table gradient through packed 2 x fp16 atomics (hash_encode(f16_from=...)) against the fp32 atomics: the dense levels
    (fp32 either way) equal to atomics order, the hashed levels to fp16 rounding of each run's contribution (2^-11 relative per term) -- relative L2 of
    the whole table below 1e-3 at gradient scales from 1e-9 to 1e+3 (the per-launch scale), d/dx untouched; and against the CPU oracle."""
    from lab4d_amd import hashgrid
    from oracle import hashgrid_oracle as HO
    L, F, log2_T, n_min, n_max, S = 16, 2, 14, 16, 512, 20000
    g = torch.Generator().manual_seed(3)
    res_l = hashgrid.level_resolutions(L, n_min, n_max)
    l16 = hashgrid.first_hashed_level(res_l, log2_T)
    assert 0 < l16 < L
    res = torch.tensor(res_l, dtype=torch.int32, device=DEV)
    table = (torch.randn(L, 1 << log2_T, F, generator=g) * 0.1).to(DEV)
    x = torch.rand(S, 3, generator=g).to(DEV)
    for mag in (1e-9, 1.0, 1e3):
        cot = (torch.randn(S, L * F, generator=g) * mag).to(DEV)
        out = []
        for f16_from in (None, l16):
            t = table.clone().requires_grad_(True)
            xx = x.clone().requires_grad_(True)
            e = hashgrid.hash_encode(xx, t, res, log2_T, f16_from=f16_from)
            gt, gx = torch.autograd.grad((e * cot).sum(), [t, xx])
            out.append((gt, gx))
        (g32, gx32), (g16, gx16) = out
        assert float((gx32 - gx16).abs().max()) <= 1e-5 * float(gx32.abs().max())  # (two kernels: the same d/dx sum of 128 terms, contracted differently)
        dense = (g16[:l16] - g32[:l16]).norm() / g32[:l16].norm()
        hashed = (g16[l16:] - g32[l16:]).norm() / g32[l16:].norm()
        assert float(dense) < 1e-6 and float(hashed) < 1e-3, (mag, float(dense), float(hashed))
        assert bool(torch.isfinite(g16).all())
    # against the oracle (a subset of the points: the oracle is a Python loop over levels)
    n_ref = 2000
    t = table.clone().requires_grad_(True)
    e = hashgrid.hash_encode(x[:n_ref], t, res, log2_T, f16_from=l16)
    cot = torch.randn(n_ref, L * F, generator=g).to(DEV)
    (gt,) = torch.autograd.grad((e * cot).sum(), [t])
    tr = table.cpu().clone().requires_grad_(True)
    er = HO.hash_encode(x[:n_ref].cpu(), tr, res_l, log2_T)
    (gr,) = torch.autograd.grad((er * cot.cpu()).sum(), [tr])
    assert float((gt.cpu() - gr).norm() / gr.norm()) < 1e-3
    # a second call reuses the scratch words the flush cleared: same result
    t2 = table.clone().requires_grad_(True)
    (gt2,) = torch.autograd.grad((hashgrid.hash_encode(x[:n_ref], t2, res, log2_T, f16_from=l16) * cot).sum(), [t2])
    assert float((gt2 - gt).norm() / gt.norm()) < 1e-3
