"""Cases and float64 references for the weight-gradient entry points lab4d_mlp_wgrad / lab4d_mlp_wgrad_mapped (csrc/mlp.hip).

Operands are drawn on the CPU, rounded to the storage type of the case (so fp32 and bf16 runs hand the device exactly the numbers the
reference sees) and laid out in the kernels' blocked buffers with NaN in the skew gaps.  Truth is the float64 product dz @ [emb; prev]^T with
the row sums of dz and the per-frame row sums over s < S; `e_ref` is the same in float32 on the CPU, in the metric the device is held to:
relative L2 of the whole tensor and of its worst 32 x 32 tile (a whole-matrix error alone would hide one wrong tile).  Everything here runs
without a GPU: tests/test_wgrad_cases_cpu.py re-asserts the reference's own error and the coverage of the case lists,
tests/test_gpu_mlp_wgrad.py runs the device against the same (cached, never modified) references."""
import functools
import os
import re
from collections import namedtuple

import torch

from lab4d_amd import mlp
from parity_report import NORTH_STAR_TOL
from raypath_cases import E_REF_MAX, REF_FACTOR, bound, gen, rel_l2  # noqa: F401  (one metric, one bound for both families of tests)

F32, BF16 = mlp.PREC_F32, mlp.PREC_BF16
PRECS = (F32, BF16)
PREC_NAME = {F32: "f32", BF16: "bf16"}
TILE = 32
NET_ID = {n.name: n.id for n in mlp.NETS}

# name; (net, layer); precision; samples; per-frame output: pf = pf_db is given, (spf, M) its frames (M = 0: refused);
# prefill = dW / db start from non-zero values; mapped = lab4d_mlp_wgrad_mapped with the layer's real column map
WgradCase = namedtuple("WgradCase", "name net layer prec S spf M pf prefill mapped")


def s_pad_of(S):
    return mlp.s_pad_of(S)


def layer_of(case):
    return mlp.describe(case.net).layers[case.layer]


def shape_of(L):
    return (L.mout_pad, L.ke, L.kin)


@functools.lru_cache(maxsize=None)
def all_layers():
    """[(net, layer, shape, pf_bias)] over every layer of every network."""
    out = []
    for n in mlp.NETS:
        d = mlp.describe(n.id)
        out += [(n.id, l, shape_of(d.layers[l]), bool(d.layers[l].pf_bias)) for l in range(d.n_layers)]
    return out


def first_layer_with(shape, pf=None):
    for net, l, sh, p in all_layers():
        if sh == shape and (pf is None or p == pf):
            return net, l
    raise KeyError(shape)


def _case(net, layer, prec, S, pf=None, prefill=False, mapped=False, tag=""):
    spf, M = pf if pf else (s_pad_of(S) if S else 256, 1)
    name = "%s%s_l%d_%s_s%d" % (tag, mlp.NET_NAMES[net], layer, PREC_NAME[prec], S)
    if pf:
        name += "_spf%d_m%d" % (spf, M)
    return WgradCase(name, net, layer, prec, S, spf, M, bool(pf), prefill, mapped)


def distinct_shapes():
    seen = []
    for _, _, sh, _ in all_layers():
        if sh not in seen:
            seen.append(sh)
    return seen


# 1. every layer shape: S = 1100 -> S_pad = 1280 = chunks of 1024 + 256
SHAPE_S = 1100
SHAPE_CASES = [_case(*first_layer_with(sh), prec, SHAPE_S) for sh in distinct_shapes() for prec in PRECS]

# 2. accumulation onto non-zero dW / db: a head, a 128-row ring, a 256-row layer
ACCUM_SHAPES = ((32, 0, 256), (128, 64, 128), (256, 0, 256))
ACCUM_CASES = [_case(*first_layer_with(sh), prec, 300, prefill=True, tag="accum_") for sh in ACCUM_SHAPES for prec in PRECS]

# 3. sizes, one shape per kernel family: the head with a short B operand (K = 64 of the 128 columns of k_mlp_wgrad_dma<1,2>), the 64-row ring
#    with half a B block (ke = 32), a 128-row ring whose B operand spans embedding and activation, the 256-row skip layer (K = 320)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1024, 1025, 2100)
SIZE_SHAPES = ((32, 0, 64), (64, 32, 0), (128, 64, 128), (256, 64, 256))
SIZE_CASES = [_case(*first_layer_with(sh), prec, S, tag="size_") for sh in SIZE_SHAPES for prec in PRECS for S in SIZES]
ZERO_CASES = [_case(*first_layer_with((128, 64, 128)), prec, 0, tag="zero_") for prec in PRECS]

# 4. / 5. per-frame bias gradient on the pf_bias layer shapes: (M, spf, S)
PF_FOLDED = ((2, 1280, 2460), (3, 256, 300), (4, 256, 1024))     # spf % 256 == 0: folded into the GEMM, chunks laid out per frame
PF_UNFOLDED = ((3, 700, 2100), (3, 1500, 4300), (1, 5000, 4100))  # k_rowsum_pf as a second pass


def pf_shapes():
    seen = []
    for _, _, sh, pf in all_layers():
        if pf and sh not in seen:
            seen.append(sh)
    return seen


def _pf_cases(triples, tag):
    return [_case(*first_layer_with(sh, pf=True), prec, S, pf=(spf, M), tag=tag) for sh in pf_shapes() for prec in PRECS for M, spf, S in triples]


PF_FOLDED_CASES = _pf_cases(PF_FOLDED, "fold_")
PF_UNFOLDED_CASES = _pf_cases(PF_UNFOLDED, "rowsum_")

# 6. mapped mode with the layers' real column maps
MAPPED_LAYERS = (("fg_base", 0), ("fg_base", 4), ("fg_color", 3), ("fg_color", 4), ("feat", 5), ("skin", 0))
MAPPED_S = 300
MAPPED_CASES = [_case(NET_ID[n], l, prec, MAPPED_S, mapped=True, tag="mapped_") for n, l in MAPPED_LAYERS for prec in PRECS]
# ... and with the per-frame table folded in (it keeps mout_pad columns, db stays untouched): a real pf_bias layer, and a head with mout < mout_pad
MAPPED_PF_CASES = [_case(NET_ID[n], l, prec, MAPPED_S, pf=(256, 2), mapped=True, tag="mapped_") for n, l in (("fg_base", 0), ("fg_color", 4))
                   for prec in PRECS]

GEMM_CASES = SHAPE_CASES + ACCUM_CASES + SIZE_CASES + PF_FOLDED_CASES + PF_UNFOLDED_CASES
ALL_CASES = GEMM_CASES + MAPPED_CASES + MAPPED_PF_CASES

# 7. host refusals: (name, what to break); the rest is a valid launch of REFUSAL_CASE
REFUSAL_CASE = _case(NET_ID["fg_base"], 4, F32, 100, tag="refuse_")
REFUSALS = ("bad_layer", "negative_layer", "null_dz", "null_dW", "null_emb", "null_act_prev", "s_pad_not_64", "s_pad_below_s", "map_without_ld_ref",
            "precision_7", "pf_unfolded_m0", "pf_unfolded_frames_short_of_s")


# ---------------------------------------------------------------------------------------------------
# the dispatch of csrc/mlp.hip, in Python
# ---------------------------------------------------------------------------------------------------


def kernel_name(case):
    return mlp.wgrad_kernel_name(layer_of(case), case.prec)


def folded(case):
    """fold_pf of lab4d_mlp_wgrad_mapped."""
    return bool(case.pf and case.spf % 256 == 0 and case.M > 0 and case.M * case.spf >= case.S)


def launch_plan(case, head_dma=True):
    """(chunk, nchunks, cpf) as lab4d_mlp_wgrad_mapped derives them (LAB4D_WGRAD_JOBS unset)."""
    L = layer_of(case)
    div_up = lambda a, b: (a + b - 1) // b
    S_pad = s_pad_of(case.S)
    mo_tiles, Kt = L.mout_pad // 32, L.ke + L.kin
    nk_tiles = Kt // 32
    big = mo_tiles >= 8
    dma = case.prec == BF16 and (mo_tiles in (8, 4, 2) or (mo_tiles == 1 and head_dma and Kt <= 256))
    if dma and mo_tiles == 1:
        nbw = 2 if Kt <= 128 else 4
    else:
        nbw = 1 if Kt <= 64 else 2 if Kt <= 128 else 3 if Kt <= 192 else 4 if Kt <= 256 else (5 if mo_tiles == 8 and Kt <= 320 else 3)
    TM = 4 if mo_tiles >= 4 else (2 if mo_tiles >= 2 else 1)
    ob_n = 1 if dma else (div_up(mo_tiles, 8) if big else div_up(mo_tiles, TM))
    kb_n = div_up(Kt, 64 * nbw) if dma else (div_up(nk_tiles, 8) if big else div_up(nk_tiles, 4))
    jobs_target = 512 if (dma and mo_tiles < 8) else 256
    nchunks = max(1, jobs_target // (ob_n * kb_n))
    chunk = max(1024, div_up(div_up(S_pad, nchunks), 256) * 256)
    if folded(case):
        chunk = min(chunk, case.spf)
        cpf = div_up(case.spf, chunk)
        return chunk, cpf * case.M, cpf
    return chunk, div_up(S_pad, chunk), 0


def chunk_formula_in_source():
    """The two lines of csrc/mlp.hip launch_plan mirrors, so that a change there fails the CPU census instead of silently moving the chunk edge."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(mlp.__file__)), "csrc", "mlp.hip")).read()
    return (re.search(r"int chunk = div_up\(div_up\(S_pad, nchunks\), 256\) \* 256; if \(chunk < 1024\) chunk = 1024;", src) is not None
            and re.search(r"jobs_target = jobs_env > 0 \? jobs_env : \(\(dma && mo_tiles < 8\) \? 512 : 256\);", src) is not None)


# ---------------------------------------------------------------------------------------------------
# blocked buffers
# ---------------------------------------------------------------------------------------------------


def block_stride(F):
    return F * 64 + 128


def to_blocked(mat, dtype=torch.float32):
    """(F, S_pad) -> the kernels' blocked buffer: element (f, s) at (s // 64) * (F * 64 + 128) + f * 64 + s % 64; the 128-element skew gap
    behind every block holds NaN."""
    F, S_pad = mat.shape
    assert S_pad % 64 == 0
    nb = S_pad // 64
    buf = torch.full((nb, block_stride(F)), float("nan"), dtype=dtype)
    buf[:, :F * 64] = mat.reshape(F, nb, 64).permute(1, 0, 2).reshape(nb, F * 64).to(dtype)
    buf = buf.reshape(-1)
    assert buf.numel() == mlp.buf_numel(F, S_pad)
    return buf


def from_blocked(buf, F, S_pad):
    """The inverse of to_blocked: (F, S_pad), the gaps dropped."""
    nb = S_pad // 64
    return buf.reshape(nb, block_stride(F))[:, :F * 64].reshape(nb, F, 64).permute(1, 0, 2).reshape(F, S_pad)


def gap_mask(F, S_pad):
    m = torch.zeros(S_pad // 64, block_stride(F), dtype=torch.bool)
    m[:, F * 64:] = True
    return m.reshape(-1)


# ---------------------------------------------------------------------------------------------------
# operands, truth, metric
# ---------------------------------------------------------------------------------------------------


def _seed(case):
    L = layer_of(case)
    return 9000 + 131 * L.mout_pad + 17 * L.ke + 3 * L.kin + 7 * case.S + 5 * case.prec + 11 * case.spf + case.M + 2 * case.prefill + case.mapped


def operands(case):
    """float32 CPU matrices (features, S_pad), already rounded to the case's storage type: dz with about half exact zeros (as after ReLU), zero on
    the padded samples S .. S_pad (the dgrad chain's contract) and non-zero on the padded rows mout .. mout_pad; a non-negative activation and
    an embedding that are finite and non-zero everywhere, the padded samples included (the forward recomputes the last sample there)."""
    L = layer_of(case)
    S, S_pad = case.S, s_pad_of(case.S)
    g = gen(_seed(case))
    q = lambda t: t.to(mlp.store_dtype(case.prec)).float()
    dz = torch.randn(L.mout_pad, S_pad, generator=g) * (torch.rand(L.mout_pad, S_pad, generator=g) < 0.5)
    dz[:, S:] = 0
    emb = prev = None
    if L.ke:
        emb = torch.rand(L.ke, S_pad, generator=g) * 2 - 1
        emb = q(torch.where(emb.abs() < 1e-3, torch.full_like(emb, 0.5), emb))
    if L.kin:
        prev = q(torch.rand(L.kin, S_pad, generator=g) + 0.01)
    return {"dz": q(dz), "emb": emb, "prev": prev}


def prefill_of(case):
    """What dW / db hold before the launch (zeros unless the case pre-fills)."""
    L = layer_of(case)
    g = gen(_seed(case) + 1)
    K = L.ke + L.kin
    if case.prefill:
        return {"dW": torch.randn(L.mout_pad, K, generator=g) * 3, "db": torch.randn(L.mout_pad, generator=g) * 3}
    return {"dW": torch.zeros(L.mout_pad, K), "db": torch.zeros(L.mout_pad)}


def _tiles(sq):
    """Sums of a non-negative matrix over its 32 x 32 tiles (ragged edges are tiles of their own)."""
    R, C = sq.shape
    pr, pc = (-R) % TILE, (-C) % TILE
    sq = torch.nn.functional.pad(sq, (0, pc, 0, pr))
    return sq.reshape((R + pr) // TILE, TILE, (C + pc) // TILE, TILE).sum((1, 3))


def worst_tile(a, truth):
    """The largest ||a - truth|| / ||truth|| over the 32 x 32 tiles of a matrix (a vector is one row of 32-element tiles); a tile whose truth
    vanishes counts 0 when a vanishes there too and inf otherwise.  NaN anywhere gives inf."""
    a, truth = a.detach().double().cpu(), truth.detach().double()
    if a.dim() == 1:
        a, truth = a[None], truth[None]
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    d, n = _tiles((a - truth) ** 2).sqrt(), _tiles(truth ** 2).sqrt()
    r = torch.where(n > 0, d / n.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(r.max())


def errors(a, truth):
    """(relative L2 of the whole tensor, of its worst tile)."""
    e = rel_l2(a, truth)
    return (e if e == e else float("inf")), worst_tile(a, truth)


def _products(ops, case, dtype):
    L = layer_of(case)
    dz = ops["dz"].to(dtype)
    X = torch.cat([t.to(dtype) for t in (ops["emb"], ops["prev"]) if t is not None], 0)
    pre = prefill_of(case)
    out = {"dW": pre["dW"].to(dtype) + dz @ X.t(), "db": pre["db"].to(dtype) + dz.sum(1)}
    if case.pf and case.M > 0:
        out["pf_db"] = torch.stack([dz[:, m * case.spf:max(m * case.spf, min((m + 1) * case.spf, case.S))].sum(1) for m in range(case.M)])
        assert out["pf_db"].shape == (case.M, L.mout_pad)
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """(truth64, e_ref): name -> float64 tensor in kernel layout (dW (mout_pad, K), db (mout_pad), pf_db (M, mout_pad)) and name ->
    (whole-tensor, worst-tile) error of the float32 CPU product.  Cached; callers must not modify it."""
    ops = operands(case)
    truth = _products(ops, case, torch.float64)
    ref32 = _products(ops, case, torch.float32)
    return truth, {k: errors(ref32[k], truth[k]) for k in truth}


# ---------------------------------------------------------------------------------------------------
# mapped mode
# ---------------------------------------------------------------------------------------------------

MAPPED_EXTRA_LD = 5   # ld_ref beyond the reference width
MAPPED_FRONT = 32     # canary elements in front of the gradient buffer inside its allocation (and at least as many behind it)
CANARY = -7.0


def column_map(case):
    return mlp.col_map(case.net, case.layer, "cpu")


def ref_width(case):
    """Columns of the reference weight: everything the column map reaches and the conditioning block next to it."""
    bd = mlp.bindings(case.net)[case.layer]
    w = int(column_map(case).max()) + 1
    return max(w, bd.cond[0] + bd.cond[1]) if bd.cond else w


def to_reference_layout(case, dWk):
    """(mout, mapped columns) of a kernel-layout matrix, and the reference columns they land in."""
    cm = column_map(case)
    keep = torch.nonzero(cm >= 0).flatten()
    return dWk[:layer_of(case).mout][:, keep], cm[keep].long()
