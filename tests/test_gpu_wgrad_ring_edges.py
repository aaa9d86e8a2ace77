"""The edges of the LDS-DMA ring of k_mlp_wgrad_dma (csrc/mlp.hip): sample ranges shorter than, equal to and just longer than the ring, held to
the float64 product.

A workgroup streams its sample range through a ring of NSTAGE 32-sample stages: a prologue that issues up to NSTAGE - 1 stages, a steady
state that refills one buffer per stage, and a drain whose counted waits shrink with the stages left.  Which of these a launch runs depends on
N, the stages in a workgroup's range.  A range is a whole number of 64-sample blocks (the entry point refuses S_pad % 64 != 0, chunks are
multiples of 256 samples, folded frames too), so N is EVEN: the odd counts 1, NSTAGE - 1 and NSTAGE + 1 (NSTAGE = 4) cannot occur.  The
cases below run every reachable N from 2 to 2 NSTAGE + 2 (one workgroup, S_pad = 64 ... 64 (NSTAGE + 1), passed directly), which brackets
each of N = 1, 2, NSTAGE - 2, NSTAGE - 1, NSTAGE, NSTAGE + 1, 2 NSTAGE + 1; a launch whose last workgroup is one block long behind a full
1024-sample chunk; and per-frame launches (spf = 256, the shortest frame the fold takes) whose every workgroup has 8 stages.

Operands are random bf16 with about half exact zeros in dz and in the activation (post-ReLU).  Truth is the float64 dz X^T and the row sums of
dz on the same bf16 values; the bound is the one of tests/test_gpu_mlp_wgrad.py: e_dev < max(1e-4, 2 e_ref) on the whole tensor and on its
worst 32 x 32 tile, e_ref the float32 CPU product's distance from the same truth."""
import functools
import os
import re

import pytest
import torch

import wgrad_cases as WC
from lab4d_amd import mlp

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = WC.CANARY
GUARD = WC.MAPPED_FRONT
# (mout, ke, kin) of the issue; the head has mout = 3 in a 32-row tile
SHAPES = ((256, 0, 256), (256, 64, 256), (256, 96, 0), (256, 64, 0), (128, 0, 128), (3, 0, 128))


@functools.lru_cache(maxsize=None)
def layer_with(shape):
    mout, ke, kin = shape
    for n in mlp.NETS:
        d = mlp.describe(n.id)
        for l in range(d.n_layers):
            L = d.layers[l]
            if (L.mout, L.ke, L.kin) == shape or (mout % 32 == 0 and (L.mout_pad, L.ke, L.kin) == shape):
                return n.id, l
    raise KeyError(shape)


def nstage(L):
    """NSTAGE of the instance that serves layer L, by the kernel's own rule."""
    K = L.ke + L.kin
    if L.mout_pad == 32:
        nbw = 2 if K <= 128 else 4
    else:
        nbw = 1 if K <= 64 else 2 if K <= 128 else 3 if K <= 192 else 4 if K <= 256 else 5
    stage = (L.mout_pad // 32) * 2048 + nbw * 4096
    return min(8, max(4, 65536 // stage))


def test_nstage_rule_is_the_one_in_the_source():
    src = open(os.path.join(os.path.dirname(os.path.abspath(mlp.__file__)), "csrc", "mlp.hip")).read()
    assert re.search(r"A_BYTES = MT \* 2048, STAGE = A_BYTES \+ NBW \* 4096;", src)
    assert re.search(r"NS0 = 65536 / STAGE, NSTAGE = NS0 < 4 \? 4 : \(NS0 > 8 \? 8 : NS0\);", src)
    assert [nstage(mlp.describe(n).layers[l]) for n, l in map(layer_with, SHAPES)] == [4, 4, 4, 4, 4, 6]


@functools.lru_cache(maxsize=None)
def problem(shape, S_pad, spf, M):
    """Operands (CPU float32 holding bf16 values), truth64 and e_ref of one launch.  Cached; never modified."""
    net, layer = layer_with(shape)
    L = mlp.describe(net).layers[layer]
    S = S_pad - 3  # the padded samples carry a zero dz and non-zero X
    g = WC.gen(77000 + 131 * L.mout_pad + 17 * L.ke + 3 * L.kin + 7 * S_pad + 11 * spf + M)
    q = lambda t: t.to(torch.bfloat16).float()
    dz = q(torch.randn(L.mout_pad, S_pad, generator=g) * (torch.rand(L.mout_pad, S_pad, generator=g) < 0.5))
    dz[:, S:] = 0
    emb = q(torch.rand(L.ke, S_pad, generator=g) * 2 - 1) if L.ke else None
    prev = q(torch.relu(torch.randn(L.kin, S_pad, generator=g))) if L.kin else None
    X = torch.cat([t for t in (emb, prev) if t is not None], 0)

    def products(dt):
        out = {"dW": dz.to(dt) @ X.to(dt).t()}
        if M:
            out["pf_db"] = torch.stack([dz[:, m * spf:(m + 1) * spf].to(dt).sum(1) for m in range(M)])
        else:
            out["db"] = dz.to(dt).sum(1)
        return out

    truth = products(torch.float64)
    ref32 = products(torch.float32)
    return (net, layer, S, dz, emb, prev), truth, {k: WC.errors(ref32[k], truth[k]) for k in truth}


def guarded(shape):
    n = 1
    for d in shape:
        n *= d
    whole = torch.full((n + 2 * GUARD,), FILL, device=DEV)
    whole[GUARD:GUARD + n] = 0
    return whole, whole[GUARD:GUARD + n].view(shape)


def run(shape, S_pad, spf=0, M=0):
    from lab4d_amd import _lib
    (net, layer, S, dz, emb, prev), truth, e_ref = problem(shape, S_pad, spf, M)
    L = mlp.describe(net).layers[layer]
    bl = lambda t: None if t is None else WC.to_blocked(t, torch.bfloat16).to(DEV)
    wW, dW = guarded((L.mout_pad, L.ke + L.kin))
    wb, db = guarded((L.mout_pad,))
    wp, pf = guarded((M, L.mout_pad)) if M else (None, None)
    if M:
        db.fill_(FILL)  # folded: the launch leaves db alone
    _lib.call("mlp_wgrad", net, layer, mlp.PREC_BF16, S, S_pad, S_pad, spf if M else S_pad, bl(dz), bl(emb), bl(prev), dW, db, pf, M)
    torch.cuda.synchronize()
    for w, t in ((wW, dW), (wb, db), (wp, pf)):
        if w is not None:
            assert bool((w[:GUARD] == FILL).all()) and bool((w[GUARD + t.numel():] == FILL).all()), "written outside an output"
    out = {"dW": dW.cpu()}
    if M:
        assert bool((db == FILL).all())
        out["pf_db"] = pf.cpu()
    else:
        out["db"] = db.cpu()
    return out, truth, e_ref


def hold(name, out, truth, e_ref):
    res = {k: WC.errors(v, truth[k]) + e_ref[k] for k, v in out.items()}
    print(name, {k: "%.2e %.2e | %.2e %.2e" % v for k, v in res.items()})
    bad = {k: v for k, v in res.items() if not (v[0] < WC.bound(v[2]) and v[1] < WC.bound(v[3]))}
    assert not bad, "%s: (e_dev, worst-tile e_dev, e_ref, worst-tile e_ref) %s" % (name, bad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d+%d" % s)
def test_one_workgroup_with_every_stage_count_around_the_ring(shape):
    L = mlp.describe(layer_with(shape)[0]).layers[layer_with(shape)[1]]
    ns = nstage(L)
    assert mlp.wgrad_kernel_name(L, mlp.PREC_BF16).startswith("k_mlp_wgrad_dma<")
    for blocks in range(1, ns + 2):  # N = 2 * blocks stages = 2 ... 2 NSTAGE + 2
        S_pad = 64 * blocks
        hold("%s N=%d" % (shape, 2 * blocks), *run(shape, S_pad))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d+%d" % s)
def test_short_last_workgroup_behind_a_full_chunk(shape):
    # chunks of 1024 samples (32 stages) and a last workgroup of one block (2 stages); 2112: two full chunks and one block
    for S_pad in (1024 + 64, 2048 + 64):
        hold("%s S_pad=%d" % (shape, S_pad), *run(shape, S_pad))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d+%d" % s)
def test_per_frame_ranges_of_eight_stages(shape):
    # spf = 256: every workgroup streams one frame of 4 blocks = 8 stages (2 NSTAGE; NSTAGE + 2 on the heads' ring of 6) into its own pf_db row
    hold("%s spf=256 M=3" % (shape,), *run(shape, 768, spf=256, M=3))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d+%d" % s)
def test_single_workgroup_per_column_block_is_deterministic(shape):
    # 576 samples = 18 stages in ONE chunk: each dW element is added once by one workgroup, so no atomic order is left to vary
    a, truth, e_ref = run(shape, 576)
    b, _, _ = run(shape, 576)
    hold("%s S_pad=576" % (shape,), a, truth, e_ref)
    assert torch.equal(a["dW"], b["dW"]) and torch.equal(a["db"], b["db"])
