"""Multiresolution hash encoding (Mueller et al. 2022) on the gfx950 kernels of csrc/hashgrid.hip -- BASELINE config 5's
encoding variant.  The reference has no such module (lab4d/nnutils/nerf.py:98 is a TODO), so this mirrors no reference
interface; it is shaped like `PosEmbedding.forward` (embedding.py:69-125: (..., 3) -> (..., C)) so that it can stand in front of
a basefield.  Parity is unpinned against the reference; the arithmetic is checked against oracle/hashgrid_oracle.py.
"""
import math

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib


def level_resolutions(L, n_min, n_max):
    """N_l = floor(N_min * b^l), b = exp((ln N_max - ln N_min) / (L - 1))  (paper eq. 2-3)."""
    b = math.exp((math.log(n_max) - math.log(n_min)) / (L - 1)) if L > 1 else 1.0
    return [int(math.floor(n_min * b ** l + 1e-9)) for l in range(L)]


_G16 = {}


def first_hashed_level(res_list, log2_T):
    """Index of the first level whose (res + 1)^3 vertices do not fit the table (hashgrid_math.hpp vertex_index): the levels in front of it are
    direct-indexed (dense), it and the finer ones go through the spatial hash."""
    for l, r in enumerate(res_list):
        if (int(r) + 1) ** 3 > (1 << log2_T):
            return l
    return len(res_list)


class _HashEncode(Function):
    @staticmethod
    def forward(ctx, x, table, res, log2_T, inside_only=False, f16_from=None, radius=None, w_min=0.0):
        x, table = x.contiguous().float(), table.contiguous().float()
        _lib.require_device(x, table, res, radius)
        S, (L, T, F) = x.shape[0], table.shape
        if T != 1 << log2_T or res.numel() != L:
            raise RuntimeError("hash_encode: table must be (L, 2^log2_T, F) with one resolution per level")
        out = torch.empty(S, L * F, device=x.device)
        # algorithmic bytes: 8 vertices x F floats gathered per level, the point read, L*F floats written
        with _lib.timed("k_hashgrid_fwd", (0.0, 4.0 * S * (8 * L * F + 3 + L * F))):
            if radius is None:
                _lib.call("hashgrid_forward_inside" if inside_only else "hashgrid_forward", x, table, res, S, L, log2_T, F, out)
            else:
                _lib.call("hashgrid_forward_aa", x, radius, table, res, S, L, log2_T, F, w_min, int(bool(inside_only)), out)
        ctx.save_for_backward(x, table, res, radius)  # (the backward recomputes the weights from the radius)
        ctx.log2_T, ctx.f16_from, ctx.w_min = log2_T, f16_from, w_min
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, table, res, radius = ctx.saved_tensors
        none = (None,) * 6  # res, log2_T, inside_only, f16_from, radius, w_min
        S, (L, T, F) = x.shape[0], table.shape
        g = g.contiguous().float()
        g_table = torch.zeros_like(table) if ctx.needs_input_grad[1] else None
        g_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        if g_table is None and g_x is None:
            return (None, None) + none
        if g_table is not None and ctx.f16_from is not None and ctx.f16_from < L:
            # the hashed levels' table gradient through packed 2 x fp16 atomics at a per-launch power-of-two scale (include/lab4d_hashgrid.h)
            if F != 2:
                raise NotImplementedError("hash_encode: the packed fp16 table gradient needs F = 2 (two features per vertex = one 32-bit word)")
            key = (x.device, L, ctx.log2_T)
            if key not in _G16:  # persistent scratch (one per device and table shape; launches on ONE stream at a time): the flush kernel hands the words back cleared, so a launch costs no 33 MB zero-fill.  Create it OUTSIDE a hipGraph capture (bench.py's eager warm-up does): a buffer born in a graph's private pool must not be touched by eager calls.
                _G16[key] = (torch.zeros(L << ctx.log2_T, dtype=torch.int32, device=x.device), torch.zeros(1, dtype=torch.int32, device=x.device))
            g16, amax = _G16[key]
            amax.zero_()
            with _lib.timed("k_hashgrid_bwd", (0.0, 4.0 * S * (2 * 8 * L * F + 6 + L * F))):
                _lib.call("hashgrid_absmax", g, g.numel(), amax)  # (of the unweighted g: w <= 1 keeps the scale's headroom)
                if radius is None:
                    _lib.call("hashgrid_backward_f16", x, table, res, g, S, L, ctx.log2_T, int(ctx.f16_from), g_table, g16, amax, g_x)
                else:
                    _lib.call("hashgrid_backward_f16_aa", x, radius, table, res, g, S, L, ctx.log2_T, int(ctx.f16_from), ctx.w_min, g_table, g16, amax, g_x)
                _lib.call("hashgrid_flush_f16", g16, amax, L, ctx.log2_T, int(ctx.f16_from), g_table)
            return (g_x, g_table) + none
        with _lib.timed("k_hashgrid_bwd", (0.0, 4.0 * S * (2 * 8 * L * F + 6 + L * F))):  # vertices read (d/dx) and atomically added to
            if radius is None:
                _lib.call("hashgrid_backward", x, table, res, g, S, L, ctx.log2_T, F, g_table, g_x)
            else:
                _lib.call("hashgrid_backward_aa", x, radius, table, res, g, S, L, ctx.log2_T, F, ctx.w_min, g_table, g_x)
        return (g_x, g_table) + none


def level_weights(radius, res, w_min=0.0):
    """The footprint weights of hash_encode(radius=..., w_min=...) in torch ops: radius (...) float32, res the level resolutions (an int tensor or
    a list) -> (..., L) float32.  The rule of csrc/hashgrid_math.hpp level_weight, operation by operation: 1 where not radius > 0 (zero, negative,
    NaN), else w = erf(1 / (sqrt(8) * radius * res)), and 0 where w < w_min.  Multiply an unweighted encoding by
    level_weights(...).repeat_interleave(F, -1) to get the weighted one; the kernels do it in place and skip what the zeros make unnecessary."""
    r = radius.float()[..., None]
    n = torch.as_tensor(res, device=r.device).to(torch.float32)
    w = torch.erf(1.0 / (2.8284271 * r * n))
    w = torch.where(w < w_min, torch.zeros_like(w), w)
    return torch.where(r > 0, w, torch.ones_like(w))


def hash_encode(x, table, res, log2_T, inside_only=False, f16_from=None, radius=None, w_min=0.0):
    """x (..., 3) in [0,1]^3, table (L, 2^log2_T, F), res: int32 device tensor (L) from level_resolutions -> (..., L*F).
    inside_only: points outside [0,1]^3 get the zero encoding and never touch the table (a field defined on the box masks them anyway).
    f16_from: None = the table gradient through fp32 atomics (exact accumulation); an int = the levels from that index on (use first_hashed_level)
    accumulate theirs through packed 2 x fp16 atomics at a per-launch scale (F = 2): half the atomics, fp16 rounding of every run's contribution.
    radius: None = every sample is a point (the kernels above, untouched); a float32 device tensor of shape x.shape[:-1] = every sample is an
    isotropic Gaussian of that radius in the unit cube and level l is multiplied by level_weights(radius, res, w_min)[..., l] inside the kernels
    (include/lab4d_hashgrid.h): a level whose weight falls below w_min (0 <= w_min <= 1) counts as zero and is neither gathered forward nor added
    to backward.  radius carries no gradient and must not require one."""
    if radius is not None:
        if radius.requires_grad:
            raise RuntimeError("hash_encode: radius must not require grad: the footprint weights are not differentiated (pass radius.detach())")
        if radius.dtype != torch.float32 or tuple(radius.shape) != tuple(x.shape[:-1]):
            raise RuntimeError("hash_encode: radius must be float32 of shape %s, got %s %s"
                               % (tuple(x.shape[:-1]), str(radius.dtype).replace("torch.", ""), tuple(radius.shape)))
        w_min = float(w_min)
        if not 0.0 <= w_min <= 1.0:
            raise RuntimeError("hash_encode: w_min = %r outside [0, 1]" % w_min)
        radius = radius.reshape(-1).contiguous()
    out = _HashEncode.apply(x.reshape(-1, 3), table, res, log2_T, inside_only, f16_from, radius, w_min)
    return out.view(x.shape[:-1] + (out.shape[-1],))
