"""Sphere tracing of the hash field's SDF to one surface hit per ray (include/lab4d_hashtrace.h, csrc/hashtrace.hip): a ray takes steps of the
size the distance allows until |sdf| <= eps, with a bisection where the sign changes.  The rules are written down in the header and in
csrc/hashtrace_math.hpp.  The raw call: hashfield.trace_surface / render_surface build on it.  No gradients; nothing here synchronises with
the host, and the call can be captured in a hipGraph."""
import math

import torch

from . import _lib

ENC, HID = 32, 64
MISS, CONVERGED, BRACKETED, STARTS_INSIDE, OUT_OF_STEPS = range(5)  # the status codes of include/lab4d_hashtrace.h
MAX_STEPS, MAX_BISECT = 1024, 32


def _check(origin, dir, t_range, aabb, table, res, log2_T, W1, b1, w2, b2, eps, step_scale, min_step, max_steps, n_bisect):
    for name, t in (("origin", origin), ("dir", dir), ("t_range", t_range), ("aabb", aabb), ("table", table), ("res", res), ("W1", W1), ("b1", b1),
                    ("w2", w2), ("b2", b2)):
        if not torch.is_tensor(t):
            raise RuntimeError("lab4d_amd.hashtrace: %s must be a device tensor, got %s" % (name, type(t).__name__))
    for name, t in (("origin", origin), ("dir", dir)):
        if t.dtype != torch.float32 or t.ndim != 2 or t.shape[1] != 3:
            raise RuntimeError("lab4d_amd.hashtrace: %s must be float32 (R, 3), got %s %s" % (name, t.dtype, tuple(t.shape)))
    R = origin.shape[0]
    if R >= 1 << 31:
        raise RuntimeError("lab4d_amd.hashtrace: %d rays, must be below 2^31" % R)
    if dir.shape[0] != R or t_range.dtype != torch.float32 or tuple(t_range.shape) != (R, 2):
        raise RuntimeError("lab4d_amd.hashtrace: origin %s, dir %s and t_range %s %s disagree: R rays need float32 (R, 3), (R, 3) and (R, 2)"
                           % (tuple(origin.shape), tuple(dir.shape), t_range.dtype, tuple(t_range.shape)))
    if aabb.dtype != torch.float32 or tuple(aabb.shape) != (2, 3):
        raise RuntimeError("lab4d_amd.hashtrace: aabb must be float32 (2, 3), got %s %s" % (aabb.dtype, tuple(aabb.shape)))
    if table.dtype != torch.float32 or table.ndim != 3:
        raise RuntimeError("lab4d_amd.hashtrace: table must be float32 (L, 2^log2_T, F), got %s %s" % (table.dtype, tuple(table.shape)))
    L, T, F = table.shape
    if L * F != ENC or L > 32 or F > 8:
        raise RuntimeError("lab4d_amd.hashtrace: L = %d, F = %d: the geometry net is instantiated for L * F = 32 hash features (L <= 32, F <= 8)" % (L, F))
    if not 4 <= log2_T <= 24 or T != 1 << log2_T:
        raise RuntimeError("lab4d_amd.hashtrace: table has %d rows per level, log2_T = %d must lie in [4, 24] with 2^log2_T rows" % (T, log2_T))
    if res.dtype != torch.int32 or res.numel() != L:
        raise RuntimeError("lab4d_amd.hashtrace: res must be int32 (L = %d,), got %s %s" % (L, res.dtype, tuple(res.shape)))
    for name, t, shape in (("W1", W1, (HID, ENC)), ("b1", b1, (HID,)), ("w2", w2, (HID,)), ("b2", b2, (1,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise RuntimeError("lab4d_amd.hashtrace: %s must be float32 %s, got %s %s" % (name, shape, t.dtype, tuple(t.shape)))
    if not (math.isfinite(eps) and eps > 0):
        raise RuntimeError("lab4d_amd.hashtrace: eps = %r must be finite and > 0" % (eps,))
    if not 0 < step_scale <= 1:
        raise RuntimeError("lab4d_amd.hashtrace: step_scale = %r outside (0, 1]" % (step_scale,))
    if not (math.isfinite(min_step) and min_step > 0):
        raise RuntimeError("lab4d_amd.hashtrace: min_step = %r must be finite and > 0" % (min_step,))
    if not 1 <= max_steps <= MAX_STEPS:
        raise RuntimeError("lab4d_amd.hashtrace: max_steps = %d outside [1, %d]" % (max_steps, MAX_STEPS))
    if not 0 <= n_bisect <= MAX_BISECT:
        raise RuntimeError("lab4d_amd.hashtrace: n_bisect = %d outside [0, %d]" % (n_bisect, MAX_BISECT))
    _lib.require_device(origin, dir, t_range, aabb, table, res, W1, b1, w2, b2)


@torch.no_grad()
def trace(origin, dir, t_range, aabb, table, res, log2_T, W1, b1, w2, b2, eps=1e-4, step_scale=1.0, min_step=None, max_steps=128, n_bisect=8):
    """origin, dir (R,3), t_range (R,2) = [t0, t1] in the units of `dir`, aabb (2,3), table (L, 2^log2_T, F) with L * F = 32, res (L,) int32,
    W1 (64,32), b1 (64): the geometry net's first Linear, w2 (64), b2 (1): row 0 of its head -- all float32 device tensors
    -> t_hit (R,) float32, status (R,) int32 (MISS, CONVERGED, BRACKETED, STARTS_INSIDE, OUT_OF_STEPS), n_eval (R,) int32, sdf_hit (R,) float32.
    eps: the hit threshold on |sdf| in world units; step = max(step_scale * sdf, min_step) / |dir| (min_step defaults to eps); at most
    max_steps evaluations while stepping and n_bisect at a sign change.  No gradients."""
    eps, step_scale, max_steps, n_bisect = float(eps), float(step_scale), int(max_steps), int(n_bisect)
    min_step = eps if min_step is None else float(min_step)
    log2_T = int(log2_T)
    _check(origin, dir, t_range, aabb, table, res, log2_T, W1, b1, w2, b2, eps, step_scale, min_step, max_steps, n_bisect)
    R, (L, _, F) = origin.shape[0], table.shape
    dev = origin.device
    t_hit, sdf_hit = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev)
    status, n_eval = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev)
    with _lib.timed("k_hashsdf_trace"):
        _lib.call("hashsdf_trace", origin.detach(), dir.detach(), t_range.detach(), aabb.detach(), R, table.detach(), res, L, log2_T, F, W1.detach(),
                  b1.detach(), w2.detach(), b2.detach(), eps, step_scale, min_step, max_steps, n_bisect, t_hit, status, n_eval, sdf_hit)
    return t_hit, status, n_eval, sdf_hit
