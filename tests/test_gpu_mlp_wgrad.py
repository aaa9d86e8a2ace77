"""lab4d_mlp_wgrad / lab4d_mlp_wgrad_mapped (csrc/mlp.hip) called directly, against the float64 product, on every dispatch branch: every
distinct layer shape in both precisions across a chunk edge, accumulation onto non-zero outputs, the sample counts around every tile, block
and chunk edge on each kernel family, the per-frame bias gradient folded into the GEMM and as the k_rowsum_pf second pass, the mapped mode
with the layers' real column maps inside canary-filled allocations, the pre-DMA bf16 head kernel in a child process, and the host refusals.

The operands are exactly representable in the storage type (tests/wgrad_cases.py), so the kernels' only legitimate error is the order of
their fp32 sums: for dW, db and pf_db, e_dev = ||device - truth64|| / ||truth64|| < max(1e-4, 2 e_ref) on the whole tensor AND on its worst
32 x 32 tile, e_ref being the float32 CPU product's distance from the same truth (tests/test_wgrad_cases_cpu.py holds e_ref <= 5e-5, so the
bound is 1e-4).  The skew gaps of the operand buffers hold NaN, the padded samples of the embedding and the activation hold non-zero numbers
under a zero dz, and every output sits between canaries that must come back bit-unchanged."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (the child process of the head-kernel test starts from this file, not from pytest)
    sys.path.insert(0, ROOT)

import wgrad_cases as WC  # noqa: E402
from parity_report import report  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = WC.CANARY
GUARD = WC.MAPPED_FRONT
WORST = {}  # kernel name -> the worst figures seen so far in this process


class Guarded:
    """A float32 device tensor with the values of `init`, inside an allocation that holds FILL in front of and behind it."""

    def __init__(self, init):
        n = init.numel()
        self.all = torch.full((n + 2 * GUARD,), FILL, device=DEV)
        self.t = self.all[GUARD:GUARD + n].view(init.shape)
        self.t.copy_(init)
        self.n = n

    def intact(self):
        return bool((self.all[:GUARD] == FILL).all()) and bool((self.all[GUARD + self.n:] == FILL).all())


def operand_buffers(case):
    from lab4d_amd import mlp
    sdt = mlp.store_dtype(case.prec)
    return {k: (None if v is None else WC.to_blocked(v, sdt).to(DEV)) for k, v in WC.operands(case).items()}


def launch(case, bufs, dW, db, pf_db, ld_ref=0, cmap=None, **over):
    """One call of the entry point the case names, with the case's own arguments unless `over` replaces one."""
    from lab4d_amd import _lib
    S_pad = WC.s_pad_of(case.S)
    a = dict(net=case.net, layer=case.layer, prec=case.prec, S=case.S, S_pad=S_pad, ld=S_pad, spf=case.spf, dz=bufs["dz"], emb=bufs["emb"],
             prev=bufs["prev"], dW=dW, db=db, pf_db=pf_db, M=case.M, ld_ref=ld_ref, cmap=cmap)
    a.update(over)
    head = (a["net"], a["layer"], a["prec"], a["S"], a["S_pad"], a["ld"], a["spf"], a["dz"], a["emb"], a["prev"], a["dW"])
    if a["cmap"] is not None:
        _lib.call("mlp_wgrad_mapped", *head, a["ld_ref"], a["cmap"], a["db"], a["pf_db"], a["M"])
    else:
        _lib.call("mlp_wgrad", *head, a["db"], a["pf_db"], a["M"])


def run_plain(case):
    """The kernel-layout outputs of one lab4d_mlp_wgrad launch, on the CPU.  db starts from FILL where the launch must leave it alone (per-frame
    sums folded into the GEMM) and must come back bit-unchanged; it is not among the returned tensors then."""
    L = WC.layer_of(case)
    pre = WC.prefill_of(case)
    fold = WC.folded(case)
    dW = Guarded(pre["dW"])
    db = Guarded(torch.full((L.mout_pad,), FILL) if fold else pre["db"])
    pf = Guarded(torch.zeros(case.M, L.mout_pad)) if case.pf else None
    launch(case, operand_buffers(case), dW.t, db.t, pf.t if pf else None)
    torch.cuda.synchronize()
    for g, k in ((dW, "dW"), (db, "db"), (pf, "pf_db")):
        assert g is None or g.intact(), "%s: written outside %s" % (case.name, k)
    out = {"dW": dW.t.cpu()}
    if fold:
        assert bool((db.t == FILL).all()), "%s: db is touched although the per-frame sums are folded into the GEMM" % case.name
    else:
        out["db"] = db.t.cpu()
    if pf:
        out["pf_db"] = pf.t.cpu()
    return out


def measure(case, dev):
    """name -> (e_dev, worst-tile e_dev, e_ref, worst-tile e_ref) for the tensors of `dev`."""
    truth, e_ref = WC.reference(case)
    return {k: WC.errors(v, truth[k]) + e_ref[k] for k, v in dev.items()}


def hold(case, res, kernel=None):
    """Report the worst figures per kernel name, then assert e_dev < max(1e-4, 2 e_ref) on the whole tensor and on the worst tile."""
    kernel = kernel or "%s@%s" % (WC.kernel_name(case), WC.PREC_NAME[case.prec])
    w = WORST.setdefault(kernel, {"e_dev": 0.0, "ratio": 0.0, "tile_e_dev": 0.0, "tile_ratio": 0.0, "cases": 0.0})
    w["cases"] += 1
    for e_dev, t_dev, e_ref, t_ref in res.values():
        w["e_dev"], w["tile_e_dev"] = max(w["e_dev"], e_dev), max(w["tile_e_dev"], t_dev)
        w["ratio"] = max(w["ratio"], e_dev / e_ref if e_ref > 0 else 0.0)
        w["tile_ratio"] = max(w["tile_ratio"], t_dev / t_ref if t_ref > 0 else 0.0)
    report("wgrad_" + re.sub(r"[^0-9a-z]+", "_", kernel.lower()).strip("_"), w)
    print(case.name, {k: "%.2e %.2e | %.2e %.2e" % v for k, v in res.items()})
    bad = {k: v for k, v in res.items() if not (v[0] < WC.bound(v[2]) and v[1] < WC.bound(v[3]))}
    assert not bad, "%s [%s]: (e_dev, worst-tile e_dev, e_ref, worst-tile e_ref) %s" % (case.name, kernel, bad)


def _expected_outputs(case):
    return {"dW", "pf_db"} if WC.folded(case) else ({"dW", "db", "pf_db"} if case.pf else {"dW", "db"})


@pytest.mark.parametrize("case", WC.GEMM_CASES, ids=lambda c: c.name)
def test_wgrad_float64_parity(case):
    dev = run_plain(case)
    assert set(dev) == _expected_outputs(case)
    hold(case, measure(case, dev))


@pytest.mark.parametrize("case", WC.ZERO_CASES, ids=lambda c: c.name)
def test_no_samples_is_ok_and_writes_nothing(case):
    L = WC.layer_of(case)
    some = case._replace(S=100)
    outs = [Guarded(torch.full(s, FILL)) for s in ((L.mout_pad, L.ke + L.kin), (L.mout_pad,), (2, L.mout_pad))]
    for pf in (None, outs[2].t):
        launch(some, operand_buffers(some), outs[0].t, outs[1].t, pf, S=0, spf=256, M=2)
        launch(some, operand_buffers(some), outs[0].t, outs[1].t, pf, S=0, S_pad=0, ld=0, spf=100, M=2)
    torch.cuda.synchronize()
    assert all(bool((g.all == FILL).all()) for g in outs)


# ---------------------------------------------------------------------------------------------------
# mapped mode
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", WC.MAPPED_CASES + WC.MAPPED_PF_CASES, ids=lambda c: c.name)
def test_wgrad_mapped_float64_parity_and_canaries(case):
    L = WC.layer_of(case)
    truth, _ = WC.reference(case)
    fold = WC.folded(case)
    assert fold == case.pf
    cm = WC.column_map(case)
    ld_ref = WC.ref_width(case) + WC.MAPPED_EXTRA_LD
    want, rcols = WC.to_reference_layout(case, truth["dW"])
    assert len(set(rcols.tolist())) == rcols.numel() and int(rcols.max()) < WC.ref_width(case)
    # mout_pad rows are allocated, mout of them are the gradient buffer: a write to a padded row is seen, not a fault
    alloc = torch.full((GUARD + L.mout_pad * ld_ref + GUARD,), FILL)
    view = alloc[GUARD:GUARD + L.mout_pad * ld_ref].view(L.mout_pad, ld_ref)
    target = torch.zeros(L.mout_pad, ld_ref, dtype=torch.bool)
    target[:L.mout, rcols] = True
    view[target] = 0
    mask = torch.zeros(alloc.numel(), dtype=torch.bool)
    mask[GUARD:GUARD + L.mout_pad * ld_ref] = target.reshape(-1)
    alloc_d = alloc.to(DEV)
    dW = alloc_d[GUARD:GUARD + L.mout_pad * ld_ref].view(L.mout_pad, ld_ref)
    db_init = torch.full((L.mout_pad,), FILL)
    if not fold:
        db_init[:L.mout] = 0
    db = Guarded(db_init)
    pf = Guarded(torch.zeros(case.M, L.mout_pad)) if case.pf else None
    launch(case, operand_buffers(case), dW, db.t, pf.t if pf else None, ld_ref=ld_ref, cmap=cm.to(DEV))
    torch.cuda.synchronize()
    after = alloc_d.cpu()
    assert torch.equal(after[~mask], alloc[~mask]), "%s: an element outside [0, mout) x the mapped columns changed" % case.name
    assert db.intact() and (pf is None or pf.intact())
    dev = {"dW": after[GUARD:GUARD + L.mout_pad * ld_ref].view(L.mout_pad, ld_ref)[:L.mout][:, rcols]}
    ref = {"dW": want}
    if fold:
        assert bool((db.t == FILL).all()), "db is not the target when the per-frame table is"
        dev["pf_db"], ref["pf_db"] = pf.t.cpu(), truth["pf_db"]  # the table keeps its mout_pad columns
        assert float(pf.t.abs().min()) > 0 or case.S < 64
    else:
        got = db.t.cpu()
        assert torch.equal(got[L.mout:], db_init[L.mout:]), "db has mout entries: the padded rows are not written"
        assert bool((got[:L.mout] != 0).all()), "every one of the mout entries is written"
        dev["db"], ref["db"] = got[:L.mout], truth["db"][:L.mout]
    _, e_ref = WC.reference(case)
    hold(case, {k: WC.errors(dev[k], ref[k]) + e_ref[k] for k in dev})


# ---------------------------------------------------------------------------------------------------
# the bf16 pre-DMA head kernel: LAB4D_WGRAD_HEAD_DMA is read once per process
# ---------------------------------------------------------------------------------------------------

HEAD_MARK = "WGRAD_HEAD_JSON "


def _head_cases():
    return [c for c in WC.SHAPE_CASES if c.prec == WC.BF16 and WC.layer_of(c).mout_pad == 32]


def _head_child():
    assert os.environ.get("LAB4D_WGRAD_HEAD_DMA") == "0"
    out = {}
    for case in _head_cases():
        assert WC.kernel_name(case) == "k_mlp_wgrad<1>", WC.kernel_name(case)
        out[case.name] = {k: list(v) for k, v in measure(case, run_plain(case)).items()}
    print(HEAD_MARK + json.dumps(out))


def test_bf16_head_kernel_without_the_dma_ring():
    cases = _head_cases()
    assert len(cases) == 3 and {WC.layer_of(c).kin for c in cases} == {64, 128, 256}
    torch.cuda.synchronize()  # the parent holds its own context and nothing in flight while it waits
    env = dict(os.environ, LAB4D_WGRAD_HEAD_DMA="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--head-child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, "the child exited with %d:\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(HEAD_MARK)]
    assert len(lines) == 1, p.stdout[-2000:]
    got = json.loads(lines[0][len(HEAD_MARK):])
    assert set(got) == {c.name for c in cases}
    for case in cases:
        assert set(got[case.name]) == {"dW", "db"}
        hold(case, {k: tuple(v) for k, v in got[case.name].items()}, kernel="k_mlp_wgrad<1>@bf16")


# ---------------------------------------------------------------------------------------------------
# refusals: decided on the host, nothing is launched
# ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("what", WC.REFUSALS)
def test_refused_on_the_host_with_nothing_launched(what):
    from lab4d_amd import _lib, mlp
    case = WC.REFUSAL_CASE
    L = WC.layer_of(case)
    assert L.ke > 0 and L.kin > 0 and case.S == 100 and WC.s_pad_of(case.S) == 256
    bufs = operand_buffers(case)
    K = L.ke + L.kin
    outs = {"dW": Guarded(torch.full((L.mout_pad, K), FILL)), "db": Guarded(torch.full((L.mout_pad,), FILL)),
            "pf_db": Guarded(torch.full((4, L.mout_pad), FILL))}
    a = dict(dW=outs["dW"].t, db=outs["db"].t, pf_db=None)
    a.update({
        "bad_layer": dict(layer=mlp.describe(case.net).n_layers),
        "negative_layer": dict(layer=-1),
        "null_dz": dict(dz=None),
        "null_dW": dict(dW=None),
        "null_emb": dict(emb=None),
        "null_act_prev": dict(prev=None),
        "s_pad_not_64": dict(S_pad=200),
        "s_pad_below_s": dict(S_pad=64),
        "map_without_ld_ref": dict(cmap=WC.column_map(case).to(DEV), ld_ref=0),
        "precision_7": dict(prec=7),
        "pf_unfolded_m0": dict(pf_db=outs["pf_db"].t, spf=100, M=0),
        "pf_unfolded_frames_short_of_s": dict(pf_db=outs["pf_db"].t, spf=30, M=3),  # sample 90 would be filed under a fourth frame
    }[what])
    _lib.PROF = {}
    try:
        with pytest.raises(RuntimeError, match="mlp_wgrad"):
            launch(case, bufs, **a)
        torch.cuda.synchronize()
        assert all(bool((g.all == FILL).all()) for g in outs.values()), "%s: refused, yet an output was written" % what
        assert _lib.prof_summary() == {}, "a refused call launched nothing: it has no place in the per-kernel profile"
    finally:
        _lib.PROF = None


if __name__ == "__main__":
    assert sys.argv[1:] == ["--head-child"], sys.argv
    _head_child()
