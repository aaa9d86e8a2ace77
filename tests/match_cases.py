"""Cases and float64 references for FeatureNeRF.global_match on the device (csrc/match.hip).

Truth is the oracle (oracle/lab4d_oracle.py: global_match, perm = arange(K)) run on float64 tensors, gradients of (out * w).sum() by
autograd; `e_ref` is the float32 oracle's distance from it in the metric the device is held to.  That metric is relative L2 (compared in
float64 on the CPU, raypath_cases.rel_l2) for every tensor but g_logsigma: a scalar that is a cancelling sum over R K terms and swings
through zero from case to case, so that an error relative to itself says nothing.  It is judged as |x - truth| / A with
A = sum_ri |ds_ri score_ri| the un-cancelled magnitude of the sum it is (ds_ri = p_ri w_r . (xc_i - out_r), the softmax's adjoint).
Everything here runs without a GPU: tests/test_match_cases_cpu.py re-asserts the reference's own error and the coverage of the case
lists, tests/test_gpu_match.py runs the device against the same (cached, never modified) references."""
import functools
from collections import namedtuple

import torch

from oracle import lab4d_oracle as O
from parity_report import NORTH_STAR_TOL  # noqa: F401
from raypath_cases import E_REF_MAX, REF_FACTOR, bound, gen, rel_l2  # noqa: F401  (one metric, one bound for every family of parity tests)

C = 16  # feature channels
MatchCase = namedtuple("MatchCase", "name R K logsigma opposed")
TENSORS = ("out", "stats_max", "stats_sum", "g_feat_c", "g_xyz_c", "g_logsigma")
ELEMENTWISE = ("out", "g_feat_c", "g_xyz_c")  # held element by element as well
LOGSIGMAS = (0.0, 2.3, 4.6)  # exp = 1 (the initial value, feature.py:86), 10, and 99: a saturated softmax


def _case(R, K, logsigma=0.0, opposed=False):
    return MatchCase("r%dk%d_ls%s%s" % (R, K, ("%.1f" % logsigma).replace(".", "p"), "_opposed" if opposed else ""), R, K, logsigma, opposed)


K_SWEEP = [_case(130, K) for K in (1, 2, 255, 256, 257, 511, 512, 513, 768, 769, 1023, 1024)]  # 3 blocks backward, per = 44
R_SWEEP = [_case(R, 300) for R in (1, 63, 64, 65, 255, 256, 257)]                              # forward block edges; NB = 1 .. 5
MULTI_TILE = [_case(R, K) for R in (16449, 32769) for K in (257, 700)]                         # per = 65 / 129: 2 / 3 LDS tiles per block
TEMPERATURES = [_case(R, K, ls) for R, K in ((130, 513), (16449, 700)) for ls in LOGSIGMAS]
CONSTANT = [_case(R, 1) for R in (1, 257, 16449)]                                              # one candidate: the softmax is constant
# every candidate points away from every pixel feature, at the highest temperature: the row maximum of the scores is below -88.8, so
# exp(0 - max) overflows float32.  0 is the score of a padded candidate register of the backward kernel (features 0), whose softmax weight
# is then infinite: nothing of it may reach a result.  One K per instantiation, R = 130 and the multi-tile R
OPPOSED = [_case(130, K, 4.6, True) for K in (2, 257, 513, 769)] + [_case(16449, 700, 4.6, True)]
# the shapes and temperatures this kernel was first tested at (against float32 torch, in a looser metric)
FIRST_SHAPES = ((1000, 1024), (4096, 300), (5, 7), (257, 1))
FIRST = [_case(R, K, ls) for R, K in FIRST_SHAPES for ls in LOGSIGMAS[:2]]
CASES = list(dict.fromkeys(K_SWEEP + R_SWEEP + MULTI_TILE + TEMPERATURES + CONSTANT + OPPOSED + FIRST))  # (the lists overlap: each case once)
WRITTEN_CASES = (_case(130, 513), _case(16449, 700))  # a K edge, and the multi-tile backward: everything is written, nothing else is
DETERMINISM_CASE = _case(16449, 700)


def inputs(case):
    """float32 CPU leaves: L2-normalised features, xyz_c ~ 0.2 randn, the cotangent w of `out`, logsigma as the (1,) float32 parameter."""
    g = gen(7000 + 31 * case.R + 3 * case.K + int(round(10 * case.logsigma)))
    n = torch.nn.functional.normalize
    fp, fc = torch.randn(case.R, C, generator=g), torch.randn(case.K, C, generator=g)
    if case.opposed:  # features within a narrow cone around u, candidates around -u: every cosine is below -0.9
        u = n(torch.randn(1, C, generator=g), dim=-1)
        fp, fc = u + 0.04 * fp, -u + 0.04 * fc
    return {"feat_px": n(fp, dim=-1), "feat_c": n(fc, dim=-1),
            "xyz_c": torch.randn(case.K, 3, generator=g) * 0.2, "w": torch.randn(case.R, 3, generator=g),
            "logsigma": torch.tensor([case.logsigma], dtype=torch.float32)}


def run_match(fn, inp, dtype=torch.float32, device="cpu"):
    """fn(feat_px, feat_c, xyz_c, logsigma) -> out (R, 3): out and the gradients of (out * w).sum() wrt feat_c, xyz_c and logsigma, detached."""
    to = lambda t: t.to(device=device, dtype=dtype)
    fc, xc, ls = (to(inp[k]).clone().requires_grad_(True) for k in ("feat_c", "xyz_c", "logsigma"))
    out = fn(to(inp["feat_px"]), fc, xc, ls)
    g = torch.autograd.grad((out * to(inp["w"])).sum(), [fc, xc, ls])
    return {"out": out.detach(), "g_feat_c": g[0].detach(), "g_xyz_c": g[1].detach(), "g_logsigma": g[2].detach()}


def oracle_match(f, fc, xc, ls):
    return O.global_match({"logsigma": ls}, f, fc, xc, torch.arange(fc.shape[0]))


def _with_stats(res, inp, dtype):
    """Adds the contract of `stats` (include/lab4d_hip.h, 3d): the row maximum of the scores and sum_i exp(score_i - max).  -> the scores."""
    score = inp["feat_px"].to(dtype) @ inp["feat_c"].to(dtype).t() * inp["logsigma"].to(dtype).exp()
    res["stats_max"] = score.max(1)[0]
    res["stats_sum"] = (score - res["stats_max"][:, None]).exp().sum(1)
    return score


@functools.lru_cache(maxsize=None)
def reference(case):
    """(truth64, ref32, A): name -> tensor for every name of TENSORS, and the un-cancelled magnitude of g_logsigma (a float).  Cached;
    callers must not modify it."""
    inp = inputs(case)
    truth = run_match(oracle_match, inp, torch.float64)
    ref32 = run_match(oracle_match, inp, torch.float32)
    _with_stats(ref32, inp, torch.float32)
    score = _with_stats(truth, inp, torch.float64)
    p = (score - truth["stats_max"][:, None]).exp_() / truth["stats_sum"][:, None]
    w, xc = inp["w"].double(), inp["xyz_c"].double()
    # w_r . (xc_i - out_r) formed from the differences, so that it is exactly zero where the softmax is constant (K = 1: out_r = xc_0)
    gd = sum(w[:, c:c + 1] * (xc[:, c][None, :] - truth["out"][:, c:c + 1]) for c in range(3))
    A = float(p.mul_(gd).mul_(score).abs_().sum())
    return truth, ref32, A


def error(name, x, truth, A):
    """The distance of x from truth[name] in the metric of the module docstring."""
    if name != "g_logsigma":
        return rel_l2(x, truth[name])
    d = abs(float(x.detach().double().cpu()) - float(truth[name]))
    return d / A if A > 0 else (0.0 if d == 0 else float("inf"))


def dispatch(R, K):
    """What the host side of csrc/match.hip launches for (R, K), re-stated: lab4d_global_match_backward picks NB = min(256, ceil(R/64))
    blocks (match_blocks() = 256) and the instantiation k_match_bwd_cand<nct>, nct = ceil(K/256); a block walks per = ceil(R/NB) rays from
    r_begin = block * per through LDS, TR = 64 at a time; k_match_fwd has 256 rays per block and passes the candidates through LDS in
    tiles of KT = 512."""
    NB = min(256, -(-R // 64)) if R else 0
    per = -(-R // NB) if NB else 0
    return {"NB": NB, "per": per, "nct": -(-K // 256), "fwd_blocks": -(-R // 256), "fwd_ktiles": -(-K // 512),
            "tiles": -(-per // 64) if NB else 0, "tail": per % 64, "empty_blocks": sum(1 for b in range(NB) if b * per >= R),
            "short_blocks": sum(1 for b in range(NB) if b * per < R < (b + 1) * per)}
