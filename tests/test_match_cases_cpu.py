"""The references tests/test_gpu_match.py holds the device to, checked without a GPU: for every case the float64 truth is finite and the
float32 oracle sits within E_REF_MAX of it in the metric of tests/match_cases.py (so max(1e-4, 2 e_ref) is 1e-4 throughout); a census
derived from the dispatch arithmetic of csrc/match.hip pins what the case lists reach, so an edited list fails here before a GPU run
silently loses coverage; and synthetic faults of the kind the kernel could have show that the metric sees them."""
import pytest
import torch

import match_cases as MC


@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c.name)
def test_match_reference_error(case):
    truth, ref32, A = MC.reference(case)
    assert set(truth) == set(ref32) == set(MC.TENSORS)
    shapes = {"out": (case.R, 3), "stats_max": (case.R,), "stats_sum": (case.R,), "g_feat_c": (case.K, MC.C), "g_xyz_c": (case.K, 3), "g_logsigma": (1,)}
    worst = 0.0
    for k in MC.TENSORS:
        t, r = truth[k], ref32[k]
        assert t.dtype == torch.float64 and r.dtype == torch.float32 and tuple(t.shape) == tuple(r.shape) == shapes[k], (case.name, k)
        assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(r).all()), (case.name, k)
        e = MC.error(k, r, truth, A)
        assert e <= MC.E_REF_MAX, "%s %s: the float32 oracle is %.2e from the float64 oracle" % (case.name, k, e)
        worst = max(worst, e)
    assert MC.bound(worst) == MC.NORTH_STAR_TOL
    assert A >= 0 and A == A and abs(float(truth["g_logsigma"])) <= A * (1 + 1e-12)
    assert bool((truth["stats_sum"] >= 1).all()), "the row maximum contributes exp(0)"
    if case.K > 1:
        assert A > 0 and float(truth["g_feat_c"].abs().min(1)[0].min()) > 0 and float(truth["g_xyz_c"].abs().min()) > 0, \
            "every candidate row receives a gradient: a row the device left unwritten cannot pass as a zero"


@pytest.mark.parametrize("case", MC.CONSTANT, ids=lambda c: c.name)
def test_one_candidate_makes_the_softmax_constant(case):
    """K = 1: out is the candidate's point, and nothing reaches the features or the temperature -- exactly, in both precisions."""
    truth, ref32, A = MC.reference(case)
    inp = MC.inputs(case)
    assert A == 0.0
    for res, dtype in ((truth, torch.float64), (ref32, torch.float32)):
        assert torch.equal(res["out"], inp["xyz_c"].to(dtype).expand(case.R, 3))
        assert float(res["g_feat_c"].abs().max()) == 0 and float(res["g_logsigma"].abs().max()) == 0
        assert torch.equal(res["stats_sum"], torch.ones(case.R, dtype=dtype))
        assert torch.equal(res["g_xyz_c"], inp["w"].to(dtype).sum(0, keepdim=True))


def test_g_logsigma_is_the_cancelling_sum_it_is_judged_as():
    """A is the magnitude of the very sum autograd forms: sum_ri ds_ri score_ri reproduces the truth of g_logsigma."""
    for case in (MC.K_SWEEP[3], MC.TEMPERATURES[2]):
        truth, _, A = MC.reference(case)
        inp = {k: v.double() for k, v in MC.inputs(case).items()}
        score = inp["feat_px"] @ inp["feat_c"].t() * inp["logsigma"].exp()
        p = torch.softmax(score, 1)
        ds = p * (inp["w"] @ inp["xyz_c"].t() - (inp["w"] * truth["out"]).sum(-1, keepdim=True))
        assert abs(float((ds * score).sum()) - float(truth["g_logsigma"])) <= 1e-12 * A
        assert abs(float((ds * score).abs().sum()) - A) <= 1e-12 * A


def test_census_of_what_the_cases_reach():
    d = {c: MC.dispatch(c.R, c.K) for c in MC.CASES}
    assert all(c in MC.CASES for lst in (MC.K_SWEEP, MC.R_SWEEP, MC.MULTI_TILE, MC.TEMPERATURES, MC.CONSTANT, MC.FIRST) for c in lst)
    assert len({c.name for c in MC.CASES}) == len(MC.CASES)
    # the lists as the work that added them states them
    assert {(c.R, c.K, c.logsigma) for c in MC.K_SWEEP} == {(130, K, 0.0) for K in (1, 2, 255, 256, 257, 511, 512, 513, 768, 769, 1023, 1024)}
    assert {(c.R, c.K, c.logsigma) for c in MC.R_SWEEP} == {(R, 300, 0.0) for R in (1, 63, 64, 65, 255, 256, 257)}
    assert {(c.R, c.K, c.logsigma) for c in MC.MULTI_TILE} == {(R, K, 0.0) for R in (16449, 32769) for K in (257, 700)}
    assert {(c.R, c.K, c.logsigma) for c in MC.TEMPERATURES} == {(R, K, ls) for R, K in ((130, 513), (16449, 700)) for ls in (0.0, 2.3, 4.6)}
    assert {(c.R, c.K, c.logsigma) for c in MC.CONSTANT} == {(R, 1, 0.0) for R in (1, 257, 16449)}
    assert {(c.R, c.K, c.logsigma) for c in MC.FIRST} == {(R, K, ls) for R, K in ((1000, 1024), (4096, 300), (5, 7), (257, 1)) for ls in (0.0, 2.3)}
    # every instantiation of k_match_bwd_cand, and both sides of each edge of its owner stride and of the forward LDS tile
    assert {v["nct"] for v in d.values()} == {1, 2, 3, 4}
    Ks = {c.K for c in MC.CASES}
    assert Ks >= {255, 256, 257, 511, 512, 513, 768, 769, 1023, 1024, 1, 2}
    for edge in (256, 512, 768):
        assert MC.dispatch(130, edge)["nct"] + 1 == MC.dispatch(130, edge + 1)["nct"]
    assert {MC.dispatch(130, K)["nct"] for K in (513, 768)} == {3} and {v["fwd_ktiles"] for v in d.values()} == {1, 2}
    assert MC.dispatch(130, 512)["fwd_ktiles"] == 1 and MC.dispatch(130, 513)["fwd_ktiles"] == 2
    # padded candidate registers (K no multiple of 256) in every instantiation
    assert {v["nct"] for c, v in d.items() if c.K % 256} == {1, 2, 3, 4}
    # the ray loop of the backward kernel: one trip only below R = 16385; beyond it a tail tile, short and empty blocks
    assert all(v["tiles"] == 1 for c, v in d.items() if c.R <= 16384) and MC.dispatch(16385, 1)["tiles"] == 2
    multi = {c: v for c, v in d.items() if v["per"] > 64}
    assert {c.R for c in multi} == {16449, 32769}
    assert {(v["NB"], v["per"], v["tiles"], v["tail"]) for v in multi.values()} == {(256, 65, 2, 1), (256, 129, 3, 1)}
    assert all(0 < v["tail"] < 64 and v["empty_blocks"] >= 1 and v["short_blocks"] == 1 for v in multi.values())
    assert MC.dispatch(16449, 700)["empty_blocks"] == 2 and 253 * 65 < 16449 < 254 * 65
    assert {c.K for c in multi} >= {1, 257, 700} and {v["nct"] for v in multi.values()} >= {1, 2, 3}
    assert {c.logsigma for c in multi} == set(MC.LOGSIGMAS)
    # block counts: one block, and every NB up to 5; forward blocks with clamped tail threads
    assert {v["NB"] for v in d.values()} >= {1, 2, 3, 4, 5, 256}
    assert any(v["NB"] == 1 and c.R == 1 for c, v in d.items())
    assert {c.R % 256 for c in MC.CASES} >= {0, 1, 255} and {v["fwd_blocks"] for v in d.values()} >= {1, 2}
    assert {c.R for c in MC.R_SWEEP} >= {63, 64, 65}, "both sides of the 64 rays of one backward tile"
    # padded candidate registers whose softmax weight overflows float32, in every instantiation and across ray tiles
    assert {(c.R, c.K, c.logsigma) for c in MC.OPPOSED} == {(130, 2, 4.6), (130, 257, 4.6), (130, 513, 4.6), (130, 769, 4.6), (16449, 700, 4.6)}
    assert all(c.opposed and c in MC.CASES and c.K % 256 for c in MC.OPPOSED) and {d[c]["nct"] for c in MC.OPPOSED} == {1, 2, 3, 4}
    for c in MC.OPPOSED:
        m = MC.reference(c)[1]["stats_max"]
        assert m.dtype == torch.float32 and not bool(torch.isfinite((0 - m).exp()).any()), "exp(0 - max) overflows float32 on every ray"
    assert not any(c.opposed for c in MC.CASES if c not in MC.OPPOSED)
    # the raw-call tests
    assert [(c.R, c.K) for c in MC.WRITTEN_CASES] == [(130, 513), (16449, 700)] and (MC.DETERMINISM_CASE.R, MC.DETERMINISM_CASE.K) == (16449, 700)


def _device_like(truth):
    """A float32 rounding of the truth: what a faultless device could return."""
    return {k: v.float() for k, v in truth.items()}


def _passes(case, dev):
    """The verdict of tests/test_gpu_match.py on `dev` (the two rules of its docstring), with e_ref taken as met."""
    truth, _, A = MC.reference(case)
    for k in MC.TENSORS:
        if not MC.error(k, dev[k], truth, A) <= MC.NORTH_STAR_TOL:
            return False
        t = truth[k]
        if k in MC.ELEMENTWISE and float(((dev[k].double() - t).abs() - (1e-5 * float(t.abs().max()) + 1e-4 * t.abs())).max()) > 0:
            return False
    return True


def test_the_metric_sees_the_faults_it_is_there_for():
    """Synthetic perturbations of a truth, each the footprint of one way the backward kernel could be wrong."""
    case = MC.MULTI_TILE[0]  # R = 16449, K = 257
    truth, _, A = MC.reference(case)
    inp = {k: v.double() for k, v in MC.inputs(case).items()}
    assert _passes(case, _device_like(truth))
    score = inp["feat_px"] @ inp["feat_c"].t() * inp["logsigma"].exp()
    p = torch.softmax(score, 1)
    ds = p * (inp["w"] @ inp["xyz_c"].t() - (inp["w"] * truth["out"]).sum(-1, keepdim=True))
    per = MC.dispatch(case.R, case.K)["per"]
    tail = torch.arange(case.R) % per >= 64  # the rays of every block's second (1-ray) tile
    assert int(tail.sum()) == 253
    # the tail tile dropped
    dev = _device_like(truth)
    dev["g_xyz_c"] = (p[~tail].t() @ inp["w"][~tail]).float()
    dev["g_feat_c"] = ((ds[~tail].t() @ inp["feat_px"][~tail]) * inp["logsigma"].exp()).float()
    dev["g_logsigma"] = (ds[~tail] * score[~tail]).sum().reshape(1).float()
    assert not _passes(case, dev)
    for k in ("g_xyz_c", "g_feat_c"):
        assert MC.error(k, dev[k], truth, A) > MC.NORTH_STAR_TOL, k
    # one padded candidate (features 0: score 0) leaking into the g_logsigma share with a score that is not 0
    dev = _device_like(truth)
    leak = float((ds[:, 0] * 1.0).abs().sum())
    dev["g_logsigma"] = (truth["g_logsigma"] + leak).float()
    assert not _passes(case, dev)
    # the last short block (4 rays) taken for empty
    dev = _device_like(truth)
    last = torch.arange(case.R) >= 253 * per
    assert int(last.sum()) == 4
    dev["g_xyz_c"] = (p[~last].t() @ inp["w"][~last]).float()
    assert not _passes(case, dev)
