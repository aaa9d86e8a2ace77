"""The references tests/test_gpu_mlp_wgrad.py holds the weight-gradient kernels to, checked without a GPU: on every case the float64 truth is
finite and the float32 CPU product sits within E_REF_MAX of it, whole tensor and worst 32 x 32 tile (so max(1e-4, 2 e_ref) is 1e-4
throughout); the blocked-buffer helper round-trips; a census pins what the case lists reach, so a new layer shape, a new kernel instantiation
or a thinned list fails here before a GPU run silently loses coverage."""
import pytest
import torch

import wgrad_cases as WC
from lab4d_amd import mlp


@pytest.fixture(autouse=True)
def _default_dispatch(monkeypatch):
    monkeypatch.delenv("LAB4D_WGRAD_HEAD_DMA", raising=False)
    monkeypatch.delenv("LAB4D_WGRAD_JOBS", raising=False)


@pytest.mark.parametrize("case", WC.ALL_CASES, ids=lambda c: c.name)
def test_reference_error(case):
    L = WC.layer_of(case)
    truth, e_ref = WC.reference(case)
    assert set(truth) == ({"dW", "db", "pf_db"} if case.pf else {"dW", "db"})
    assert truth["dW"].shape == (L.mout_pad, L.ke + L.kin) and truth["db"].shape == (L.mout_pad,)
    for k, t in truth.items():
        assert t.dtype == torch.float64 and bool(torch.isfinite(t).all()), (case.name, k)
        whole, tile = e_ref[k]
        assert whole <= WC.E_REF_MAX and tile <= WC.E_REF_MAX, "%s %s: the float32 product is %.2e (worst tile %.2e) from the float64 one" % (case.name, k, whole, tile)
        assert WC.bound(whole) == WC.bound(tile) == WC.NORTH_STAR_TOL
    if case.S >= 64:  # every 32 x 32 tile of the truth carries signal, the padded rows included: a tile the device leaves out cannot pass
        assert float(WC._tiles(truth["dW"] ** 2).min()) > 0 and float(WC._tiles(truth["db"][None] ** 2).min()) > 0


@pytest.mark.parametrize("case", [WC.SHAPE_CASES[0], WC.SHAPE_CASES[1], WC.SIZE_CASES[0], WC.PF_UNFOLDED_CASES[1]], ids=lambda c: c.name)
def test_operands_are_what_the_cases_claim(case):
    L = WC.layer_of(case)
    S, S_pad = case.S, WC.s_pad_of(case.S)
    ops = WC.operands(case)
    dz = ops["dz"]
    assert dz.shape == (L.mout_pad, S_pad) and float(dz[:, S:].abs().max()) == 0, "dz is zero on the padded samples"
    zeros = float((dz[:, :S] == 0).float().mean())
    assert (0.3 < zeros < 0.7) if S >= 64 else True, zeros
    if S >= 64:
        assert bool((dz[L.mout:, :S].abs().sum(1) > 0).all()) or L.mout == L.mout_pad, "the padded rows of dz carry values"
    for k, rows in (("emb", L.ke), ("prev", L.kin)):
        t = ops[k]
        assert (t is None) == (rows == 0)
        if t is not None:
            assert t.shape == (rows, S_pad) and bool(torch.isfinite(t).all()) and float(t.abs().min()) > 0, k
            assert k == "emb" or float(t.min()) > 0, "the activation is non-negative"
    sdt = mlp.store_dtype(case.prec)
    for t in ops.values():
        assert t is None or torch.equal(t.to(sdt).float(), t), "exactly representable in the storage type"


def test_blocked_layout_round_trips_and_keeps_nan_to_the_gaps():
    for F, S_pad in ((32, 64), (96, 256), (256, 1280)):
        mat = torch.arange(F * S_pad, dtype=torch.float32).reshape(F, S_pad)
        buf = WC.to_blocked(mat)
        assert buf.numel() == mlp.buf_numel(F, S_pad)
        assert torch.equal(WC.from_blocked(buf, F, S_pad), mat)
        assert torch.equal(torch.isnan(buf), WC.gap_mask(F, S_pad)) and int(WC.gap_mask(F, S_pad).sum()) == 128 * (S_pad // 64)
        for f, s in ((0, 0), (F - 1, S_pad - 1), (F // 2, 63), (1, S_pad - 64)):
            assert float(buf[(s // 64) * (F * 64 + 128) + f * 64 + s % 64]) == float(mat[f, s])
    b16 = WC.to_blocked(torch.ones(32, 128), torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and int(torch.isnan(b16).sum()) == 256


def test_the_metric_sees_one_wrong_tile():
    t = torch.randn(64, 96, generator=WC.gen(1), dtype=torch.float64) * 10
    a = t.clone()
    assert WC.errors(a, t) == (0.0, 0.0)
    a[40, 70] += 0.05 * float(t[32:64, 64:96].norm())
    whole, tile = WC.errors(a, t)
    assert abs(tile - 0.05) < 1e-9 and whole < tile / 2
    a[0, 0] = float("nan")
    assert WC.errors(a, t) == (float("inf"), float("inf"))
    z = torch.zeros(32, 32, dtype=torch.float64)
    assert WC.worst_tile(z, z) == 0 and WC.worst_tile(z + 1e-9, z) == float("inf")
    v = torch.arange(1, 41, dtype=torch.float64)
    assert WC.worst_tile(v, v) == 0 and WC.worst_tile(torch.cat([v[:39], v[39:] * 2]), v) > 0.1, "a vector is tiled too, ragged edge included"


def test_census_of_what_the_cases_reach():
    assert WC.chunk_formula_in_source(), "csrc/mlp.hip no longer derives its chunk the way wgrad_cases.launch_plan does"
    every = {(net, l, prec) for net, l, _, _ in WC.all_layers() for prec in WC.PRECS}
    wanted = {(prec, mlp.wgrad_kernel_name(mlp.describe(net).layers[l], prec)) for net, l, prec in every}
    assert {(c.prec, WC.kernel_name(c)) for c in WC.SHAPE_CASES} == wanted
    dma = {n for p, n in wanted if n.startswith("k_mlp_wgrad_dma")}
    assert dma == {"k_mlp_wgrad_dma<%s>" % t for t in ("8,1", "8,2", "8,4", "8,5", "4,1", "4,2", "4,3", "4,4", "2,1", "2,2", "2,3", "1,2", "1,4")}
    assert {n for p, n in wanted if p == WC.F32} == {"k_mlp_wgrad<1>", "k_mlp_wgrad<2>", "k_mlp_wgrad<4>", "k_mlp_wgrad_big"}
    shapes = {sh for _, _, sh, _ in WC.all_layers()}
    assert len(shapes) == len(WC.distinct_shapes()) == 16
    for prec in WC.PRECS:
        assert {WC.shape_of(WC.layer_of(c)) for c in WC.SHAPE_CASES if c.prec == prec} == shapes, "every distinct (mout_pad, ke, kin)"
    # list 1 crosses a chunk edge, with a ragged last chunk
    for c in WC.SHAPE_CASES:
        chunk, nchunks, cpf = WC.launch_plan(c)
        S_pad = WC.s_pad_of(c.S)
        assert S_pad > chunk and nchunks == 2 and S_pad % chunk and cpf == 0, (c.name, chunk, nchunks)
    # sizes: every size on every family in both precisions; one, two and three chunks
    fams = {(c.prec, WC.kernel_name(c)) for c in WC.SIZE_CASES}
    assert fams == {(WC.F32, "k_mlp_wgrad<1>"), (WC.F32, "k_mlp_wgrad<2>"), (WC.F32, "k_mlp_wgrad<4>"), (WC.F32, "k_mlp_wgrad_big"),
                    (WC.BF16, "k_mlp_wgrad_dma<1,2>"), (WC.BF16, "k_mlp_wgrad_dma<2,1>"), (WC.BF16, "k_mlp_wgrad_dma<4,3>"), (WC.BF16, "k_mlp_wgrad_dma<8,5>")}
    for fam in fams:
        mine = [c for c in WC.SIZE_CASES if (c.prec, WC.kernel_name(c)) == fam]
        assert {c.S for c in mine} == {1, 63, 64, 65, 255, 256, 257, 1024, 1025, 2100}, fam
        assert {WC.launch_plan(c)[1] for c in mine} == {1, 2, 3}, fam
    assert {c.S for c in WC.ZERO_CASES} == {0} and {c.prec for c in WC.ZERO_CASES} == set(WC.PRECS)
    # short B operands of the DMA ring (K below the columns of the instantiation): half a block, and the head's 64 of 128
    short = {WC.kernel_name(c) for c in WC.SIZE_CASES if c.prec == WC.BF16 and (WC.layer_of(c).ke + WC.layer_of(c).kin) % (64 * int(WC.kernel_name(c)[-2])) != 0}
    assert short == {"k_mlp_wgrad_dma<1,2>", "k_mlp_wgrad_dma<2,1>"}
    # accumulation: a head, a 64/128-row ring, a 256-row layer
    assert {WC.layer_of(c).mout_pad for c in WC.ACCUM_CASES} == {32, 128, 256} and all(c.prefill for c in WC.ACCUM_CASES)
    assert all(float(WC.prefill_of(c)["dW"].abs().min()) > 0 and float(WC.prefill_of(c)["db"].abs().min()) > 0 for c in WC.ACCUM_CASES)
    # per-frame bias gradient: the pf_bias layer shapes, folded and not, several frames per launch
    pf_shapes = {sh for _, _, sh, pf in WC.all_layers() if pf}
    assert len(pf_shapes) == 8
    for cases, triples, fold in ((WC.PF_FOLDED_CASES, {(2, 1280, 2460), (3, 256, 300), (4, 256, 1024)}, True),
                                 (WC.PF_UNFOLDED_CASES, {(3, 700, 2100), (3, 1500, 4300), (1, 5000, 4100)}, False)):
        assert all(c.pf and WC.folded(c) == fold and mlp.describe(c.net).layers[c.layer].pf_bias for c in cases)
        for prec in WC.PRECS:
            assert {(WC.shape_of(WC.layer_of(c)), (c.M, c.spf, c.S)) for c in cases if c.prec == prec} == {(sh, t) for sh in pf_shapes for t in triples}
        assert any(c.M > 1 for c in cases), "more than one frame per launch"
    plans = {(c.M, c.spf, c.S): WC.launch_plan(c) for c in WC.PF_FOLDED_CASES}
    assert plans[(2, 1280, 2460)] == (1024, 4, 2), "cpf = 2: chunks of 1024 and 256 per frame"
    assert plans[(3, 256, 300)] == (256, 3, 1) and 2 * 256 == WC.s_pad_of(300), "the last frame starts at S_pad: an empty job"
    assert plans[(4, 256, 1024)] == (256, 4, 1)
    assert any(c.spf < 4096 < c.S and 4096 % c.spf for c in WC.PF_UNFOLDED_CASES), "the 4096-sample segment edge falls inside a frame"
    assert any(c.S > 4096 and c.M == 1 for c in WC.PF_UNFOLDED_CASES)
    # mapped mode
    names = {(mlp.NET_NAMES[c.net], c.layer) for c in WC.MAPPED_CASES}
    assert names == {("fg_base", 0), ("fg_base", 4), ("fg_color", 3), ("fg_color", 4), ("feat", 5), ("skin", 0)}
    for c in WC.MAPPED_CASES + WC.MAPPED_PF_CASES:
        assert c.mapped and {x.prec for x in WC.MAPPED_CASES if (x.net, x.layer) == (c.net, c.layer)} == set(WC.PRECS)
    by = {(mlp.NET_NAMES[c.net], c.layer): c for c in WC.MAPPED_CASES}
    cm = WC.column_map(by[("fg_base", 4)])
    assert cm.numel() == 320 and int((cm < 0).sum()) > 0 and WC.ref_width(by[("fg_base", 4)]) == 63 + 32 + 256
    assert not set(range(63, 95)) & set(cm.tolist()), "the conditioning columns have no kernel column"
    emb = WC.column_map(by[("fg_base", 0)])[:63]
    assert sorted(emb.tolist()) == list(range(63)) and emb.tolist() != list(range(63)), "a permutation of the posenc channels"
    for key in (("fg_color", 4), ("feat", 5)):
        L = WC.layer_of(by[key])
        assert L.mout < L.mout_pad == 32
    assert all(WC.folded(c) and c.M > 1 for c in WC.MAPPED_PF_CASES)
    assert {WC.layer_of(c).mout < WC.layer_of(c).mout_pad for c in WC.MAPPED_PF_CASES} == {True, False}
    assert len(WC.REFUSALS) == len(set(WC.REFUSALS)) >= 11
    assert len({c.name for c in WC.ALL_CASES}) == len(WC.ALL_CASES)
