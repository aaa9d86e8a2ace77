"""Packed ray marching and ragged compositing of the hash field (include/lab4d_packed.h, csrc/packed.hip): `march` steps every ray at a fixed
step through the occupied cells of an occgrid.OccupancyGrid and emits the kept samples of all rays as ONE packed list with a per-ray
(start, count); `composite` renders that list directly.  Nothing of size rays x samples-per-ray exists.  The reference has no counterpart
(nnutils/nerf.py:98 is a TODO); the rules are written down in the header and in csrc/packed_math.hpp.  `prune` (include/lab4d_prune.h,
csrc/prune.hip) drops the rows of such a list that lie behind the point where their ray has become opaque, and the rows without opacity,
given the density of the rows: the step between a density pass without gradients and the differentiable field.  `distortion`
(include/lab4d_distort.h, csrc/distort.hip) is the distortion loss of such a list per ray, with its adjoint.  `merge` and `merge_rows`
(include/lab4d_pmerge.h, csrc/pmerge.hip) z-sort the rows of two such lists of the same rays into one and gather per-row values through the
order: a foreground field in front of a background, composited as one list.  `weights` and `resample`
(include/lab4d_presample.h, csrc/presample.hip) are the coarse-to-fine step: the compositing weights of a list without gradients, and the
inverse-CDF resampling of the list into n_imp rows per ray where those weights are.  `render_weights` and `proposal_loss`
(include/lab4d_proposal.h, csrc/proposal.hip) train a proposal field for that step: the weights with a backward, and the interval loss
that makes a proposal list's weights an upper envelope of the fine list's.  `march_cone` (include/lab4d_conemarch.h, csrc/conemarch.hip) is
`march` with a step that grows with the distance, through a cascade of occupancy grids (occgrid.OccupancyCascade): the same packed layout
with a step and a level per row, which everything above takes as it is.  Nothing here synchronises
with the host: every call can be captured in a hipGraph."""
import collections
import math
import struct

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib


def _f32(name, t, *tail):
    _lib.require_device(t)
    if t.dtype != torch.float32 or t.ndim != len(tail) + 1 or tuple(t.shape[1:]) != tail:
        raise RuntimeError("lab4d_amd.packed: %s must be float32 (n%s), got %s %s" % (name, "".join(", %d" % x for x in tail), t.dtype, tuple(t.shape)))


class PackedRays:
    """The packed sample list of one march.  Per row (cap rows): t (cap,) the ray parameter, deltas (cap,) = dt * |dir| of the row's ray,
    xyz (cap,3), dirs (cap,3) unit view directions, ray_idx (cap,) int32.  Per ray (R): ray_start, ray_count int32 -- ray r owns rows
    ray_start[r] .. + ray_count[r], in ascending t; ray_count is cut at the capacity.  total (1,) int32: the untruncated number of kept
    samples; overflow (1,) bool: total > cap (samples were dropped).  Rows behind min(total, cap) are parked outside the box with
    ray_idx = -1, t = 0, deltas = 0."""
    __slots__ = ("t", "deltas", "xyz", "dirs", "ray_idx", "ray_start", "ray_count", "total", "overflow", "R", "cap")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


@torch.no_grad()
def march(grid, origin, dir, t_range, dt, cap, k_max=1024):
    """grid: occgrid.OccupancyGrid; origin, dir (R,3), t_range (R,2) = [t0, t1] in the units of `dir`; dt > 0 the step in those units;
    cap: the STATIC number of packed rows; k_max: at most this many candidates t0 + (k + 0.5) dt per ray.  -> PackedRays.  Two kernels
    (count, write) around one prefix sum; no read-back."""
    _f32("origin", origin, 3)
    _f32("dir", dir, 3)
    _f32("t_range", t_range, 2)
    R, dt, cap, k_max = origin.shape[0], float(dt), int(cap), int(k_max)
    if dir.shape[0] != R or t_range.shape[0] != R:
        raise RuntimeError("lab4d_amd.packed.march: origin %s, dir %s and t_range %s disagree on the number of rays"
                           % (tuple(origin.shape), tuple(dir.shape), tuple(t_range.shape)))
    if not (math.isfinite(dt) and dt > 0):
        raise RuntimeError("lab4d_amd.packed.march: dt = %r must be finite and > 0" % dt)
    if k_max < 1:
        raise RuntimeError("lab4d_amd.packed.march: k_max = %d must be >= 1" % k_max)
    if R * k_max >= 1 << 31:
        raise RuntimeError("lab4d_amd.packed.march: R * k_max = %d * %d does not fit 31 bits" % (R, k_max))
    if not 0 <= cap < 1 << 31:
        raise RuntimeError("lab4d_amd.packed.march: cap = %d outside [0, 2^31)" % cap)
    dev = origin.device
    origin, dir, t_range = origin.detach(), dir.detach(), t_range.detach()
    count = torch.empty(R, dtype=torch.int32, device=dev)
    head = [origin, dir, t_range, grid.aabb, grid.bits, grid.G, R, dt, k_max]
    _lib.call("packed_march_count", *head, count)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count  # (the exclusive scan: R * k_max < 2^31, the sums fit)
    out = {"t": torch.empty(cap, device=dev), "deltas": torch.empty(cap, device=dev), "xyz": torch.empty(cap, 3, device=dev),
           "dirs": torch.empty(cap, 3, device=dev), "ray_idx": torch.empty(cap, dtype=torch.int32, device=dev),
           "ray_count": torch.empty(R, dtype=torch.int32, device=dev), "total": torch.empty(1, dtype=torch.int32, device=dev)}
    overflow = torch.empty(1, dtype=torch.uint8, device=dev)
    _lib.call("packed_march_write", *head, start, cap, out["t"], out["deltas"], out["xyz"], out["dirs"], out["ray_idx"], out["ray_count"], out["total"],
              overflow)
    return PackedRays(ray_start=start, overflow=overflow.view(torch.bool), R=R, cap=cap, **out)


class ConeRays(PackedRays):
    """The packed list of one cone-stepped march: a PackedRays whose rows also carry steps (cap,), the row's own step s_k in the units of t
    (deltas = steps * |dir|: per row, not per ray), and level (cap,) int32, the cascade level the row was looked up in (-1 in the parked
    rows, whose steps are 0)."""
    __slots__ = ("steps", "level")

    def __init__(self, **kw):
        for k in PackedRays.__slots__ + self.__slots__:
            setattr(self, k, kw[k])


@torch.no_grad()
def march_cone(cascade, origin, dir, t_range, cone, dt_min, dt_max, cap, k_max=1024):
    """cascade: occgrid.OccupancyCascade; origin, dir (R,3), t_range (R,2) = [t0, t1] in the units of `dir`; the step grows with the ray
    parameter, s = clamp(a * cone, dt_min, dt_max) from the ray's entry into the outermost box on, each interval [a, a + s] giving one
    candidate at its middle; a candidate is kept iff its bit is set at the cascade level that fits its position and its step (rules:
    include/lab4d_conemarch.h).  cone >= 0 (0: a fixed step dt_min), 0 < dt_min <= dt_max; cap: the STATIC number of packed rows; k_max: at
    most this many candidates per ray.  -> ConeRays, accepted as it is by composite, prune, distortion, weights / resample, merge and
    render_weights / proposal_loss.  Two kernels (count, write) around one prefix sum; no read-back."""
    R, cone, dt_min, dt_max, cap, k_max = origin.shape[0], float(cone), float(dt_min), float(dt_max), int(cap), int(k_max)
    if not (math.isfinite(cone) and cone >= 0):  # (the scalars first: refused whatever the tensors are)
        raise RuntimeError("lab4d_amd.packed.march_cone: cone = %r must be finite and >= 0" % cone)
    if not (math.isfinite(dt_min) and dt_min > 0):
        raise RuntimeError("lab4d_amd.packed.march_cone: dt_min = %r must be finite and > 0" % dt_min)
    if not (math.isfinite(dt_max) and dt_max >= dt_min):
        raise RuntimeError("lab4d_amd.packed.march_cone: dt_max = %r must be finite and >= dt_min = %r" % (dt_max, dt_min))
    if k_max < 1:
        raise RuntimeError("lab4d_amd.packed.march_cone: k_max = %d must be >= 1" % k_max)
    if R * k_max >= 1 << 31:
        raise RuntimeError("lab4d_amd.packed.march_cone: R * k_max = %d * %d does not fit 31 bits" % (R, k_max))
    if not 0 <= cap < 1 << 31:
        raise RuntimeError("lab4d_amd.packed.march_cone: cap = %d outside [0, 2^31)" % cap)
    _f32("origin", origin, 3)
    _f32("dir", dir, 3)
    _f32("t_range", t_range, 2)
    if dir.shape[0] != R or t_range.shape[0] != R:
        raise RuntimeError("lab4d_amd.packed.march_cone: origin %s, dir %s and t_range %s disagree on the number of rays"
                           % (tuple(origin.shape), tuple(dir.shape), tuple(t_range.shape)))
    dev = origin.device
    origin, dir, t_range = origin.detach(), dir.detach(), t_range.detach()
    count = torch.empty(R, dtype=torch.int32, device=dev)
    head = [origin, dir, t_range, cascade.aabbs, cascade.bits, cascade.K, cascade.G, R, cone, dt_min, dt_max, k_max]
    _lib.call("packed_march_cone_count", *head, count)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count  # (the exclusive scan: R * k_max < 2^31, the sums fit)
    out = {"t": torch.empty(cap, device=dev), "steps": torch.empty(cap, device=dev), "deltas": torch.empty(cap, device=dev),
           "xyz": torch.empty(cap, 3, device=dev), "dirs": torch.empty(cap, 3, device=dev), "ray_idx": torch.empty(cap, dtype=torch.int32, device=dev),
           "level": torch.empty(cap, dtype=torch.int32, device=dev), "ray_count": torch.empty(R, dtype=torch.int32, device=dev),
           "total": torch.empty(1, dtype=torch.int32, device=dev)}
    overflow = torch.empty(1, dtype=torch.uint8, device=dev)
    _lib.call("packed_march_cone_write", *head, start, cap, out["t"], out["steps"], out["deltas"], out["xyz"], out["dirs"], out["ray_idx"], out["level"],
              out["ray_count"], out["total"], overflow)
    return ConeRays(ray_start=start, overflow=overflow.view(torch.bool), R=R, cap=cap, **out)


def _field_list(fields, modes):
    fl = _lib.FieldList()
    fl.n_fields = len(fields)
    sumC = 0
    for i, (f, m) in enumerate(zip(fields, modes)):
        fl.fields[i] = _lib.dp(f)
        fl.channels[i] = f.shape[-1]
        fl.modes[i] = m
        sumC += 1 if m == 2 else f.shape[-1]
    return fl, sumC


class _PackedComposite(Function):
    @staticmethod
    def forward(ctx, density, deltas, ray_start, ray_count, modes, *fields):
        P, R = density.shape[0], ray_start.shape[0]
        fl, sumC = _field_list(fields, modes)
        mask = torch.empty(R, 1, device=density.device)
        out = torch.empty(R, max(sumC, 1), device=density.device)
        _lib.call("packed_composite_forward", density, deltas, fl, ray_start, ray_count, R, P, None, None, mask, out)
        ctx.save_for_backward(density, deltas, ray_start, ray_count, *fields)
        ctx.modes = tuple(modes)
        return mask, out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mask, g_out):
        density, deltas, ray_start, ray_count, *fields = ctx.saved_tensors
        P, R = density.shape[0], ray_start.shape[0]
        fl, _ = _field_list(fields, ctx.modes)
        gf = _lib.FieldGrads()
        gf.n_fields = len(fields)
        gfields = []
        for i, f in enumerate(fields):
            g = torch.zeros_like(f) if ctx.needs_input_grad[5 + i] else None  # (zeros: the rows that no ray owns are not written)
            gfields.append(g)
            gf.fields[i] = _lib.dp(g) if g is not None else None
        g_density = torch.zeros_like(density) if ctx.needs_input_grad[0] else None
        g_deltas = torch.zeros_like(deltas) if ctx.needs_input_grad[1] else None
        g_mask = g_mask.contiguous() if g_mask is not None else None
        g_out = g_out.contiguous() if g_out is not None else None
        _lib.call("packed_composite_backward", density, deltas, fl, ray_start, ray_count, R, P, g_mask, g_out, g_density, g_deltas, gf)
        return (g_density, g_deltas, None, None, None, *gfields)


def composite(density, deltas, fields, rays, modes=None):
    """density, deltas (P,) or (P,1) on the packed rows of `rays` (a PackedRays, or anything with ray_start / ray_count (R,) int32);
    fields: dict name -> (P, c); modes: dict name -> 0 (weights normalised by mask + 1e-6; the default), 1 (the same, weights detached),
    2 (plain mean over the ray's samples and channels).  -> (rendered: dict name -> (R, c), or (R,) for a mode-2 field; mask (R,1)).
    A ray without samples renders zeros.  Differentiable in density, deltas and the fields."""
    names = list(fields)
    if len(names) > 16:
        raise RuntimeError("lab4d_amd.packed.composite: more than 16 fields")
    ms = [int((modes or {}).get(k, 0)) for k in names]
    if any(m not in (0, 1, 2) for m in ms):
        raise RuntimeError("lab4d_amd.packed.composite: modes are 0, 1 or 2, got %s" % ms)
    _lib.require_device(density, deltas, rays.ray_start, rays.ray_count, *fields.values())
    P = density.shape[0]
    if density.numel() != P or deltas.numel() != P or density.dtype != torch.float32 or deltas.dtype != torch.float32:
        raise RuntimeError("lab4d_amd.packed.composite: density %s and deltas %s must be float32 (P,) or (P, 1)" % (tuple(density.shape), tuple(deltas.shape)))
    fs = []
    for k in names:
        f = fields[k]
        if f.dtype != torch.float32 or f.ndim != 2 or f.shape[0] != P or not 1 <= f.shape[1] <= 64:
            raise RuntimeError("lab4d_amd.packed.composite: field %s must be float32 (%d, 1..64), got %s %s" % (k, P, f.dtype, tuple(f.shape)))
        fs.append(f)
    if sum(1 if m == 2 else f.shape[1] for f, m in zip(fs, ms)) > 64:
        raise RuntimeError("lab4d_amd.packed.composite: more than 64 output channels")
    rs, rc = rays.ray_start, rays.ray_count
    if rs.dtype != torch.int32 or rc.dtype != torch.int32 or rs.ndim != 1 or rs.shape != rc.shape:
        raise RuntimeError("lab4d_amd.packed.composite: ray_start / ray_count must be int32 (R,)")
    mask, out = _PackedComposite.apply(density.reshape(P), deltas.reshape(P), rs, rc, tuple(ms), *fs)
    rendered, co = {}, 0
    for k, m, f in zip(names, ms, fs):
        c = 1 if m == 2 else f.shape[1]
        rendered[k] = out[:, co] if m == 2 else out[:, co:co + c]
        co += c
    return rendered, mask


# ---------------------------------------------------------------------------------------------------
# pruning by transmittance and opacity (include/lab4d_prune.h, csrc/prune.hip)
# ---------------------------------------------------------------------------------------------------
class PrunedRays(PackedRays):
    """The packed list of one prune: a PackedRays (total / overflow / cap are the prune's own) that also carries src_row (cap,) int32, the
    row of the pruned list's source that every surviving row was copied from (-1 in the parked rows): what a caller gathers through to
    reuse anything it already computed per row."""
    __slots__ = ("src_row",)

    def __init__(self, **kw):
        for k in PackedRays.__slots__ + self.__slots__:
            setattr(self, k, kw[k])


def _as_f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def prune_thresholds(early_stop_eps, alpha_thre):
    """The two user-facing values in the tau domain, converted in double precision and rounded to fp32 once (the kernels never call exp):
    tau_stop = -log(early_stop_eps), +inf for 0: a ray stops where its transmittance has fallen below early_stop_eps;
    tau_min = -log1p(-alpha_thre): a row is dropped when its opacity 1 - exp(-tau) lies below alpha_thre.  Both must lie in [0, 1)."""
    eps, alpha = float(early_stop_eps), float(alpha_thre)
    if not 0.0 <= eps < 1.0:
        raise RuntimeError("lab4d_amd.packed.prune: early_stop_eps = %r outside [0, 1)" % early_stop_eps)
    if not 0.0 <= alpha < 1.0:
        raise RuntimeError("lab4d_amd.packed.prune: alpha_thre = %r outside [0, 1)" % alpha_thre)
    return (_as_f32(-math.log(eps)) if eps > 0.0 else math.inf), _as_f32(-math.log1p(-alpha))


@torch.no_grad()
def prune(rays, density, early_stop_eps=1e-4, alpha_thre=0.0, cap=None, *, aabb):
    """rays: a PackedRays; density (P,) or (P,1) float32 on its rows (detached here: the decision is not differentiable); aabb: the box
    (2,3) / (6,) float32 the list was marched in (grid.aabb) -- the park point of the rows behind the count, which a PackedRays does not
    carry.  Drops every row at and behind the first row of its ray whose transmittance in front of it, exp(-sum of tau before it), lies
    below early_stop_eps, and every row whose opacity 1 - exp(-tau) lies below alpha_thre (rules: include/lab4d_prune.h).
    -> PrunedRays with `cap` rows (default rays.cap), laid out like a march's.  Two kernels (count, write) around one prefix sum; no
    read-back."""
    tau_stop, tau_min = prune_thresholds(early_stop_eps, alpha_thre)
    cap = rays.cap if cap is None else int(cap)
    if not 0 <= cap < 1 << 31:
        raise RuntimeError("lab4d_amd.packed.prune: cap = %d outside [0, 2^31)" % cap)
    P, R = rays.t.shape[0], rays.ray_start.shape[0]
    _lib.require_device(density, aabb, rays.t, rays.deltas, rays.xyz, rays.dirs, rays.ray_start, rays.ray_count)
    if density.numel() != P or density.dtype != torch.float32 or density.ndim not in (1, 2):
        raise RuntimeError("lab4d_amd.packed.prune: density must be float32 (%d,) or (%d, 1), got %s %s" % (P, P, density.dtype, tuple(density.shape)))
    if aabb.numel() != 6 or aabb.dtype != torch.float32:
        raise RuntimeError("lab4d_amd.packed.prune: aabb must be float32 (2, 3) or (6,), got %s %s" % (aabb.dtype, tuple(aabb.shape)))
    _f32("rays.t", rays.t)
    _f32("rays.deltas", rays.deltas)
    _f32("rays.xyz", rays.xyz, 3)
    _f32("rays.dirs", rays.dirs, 3)
    rs, rc = rays.ray_start, rays.ray_count
    if rs.dtype != torch.int32 or rc.dtype != torch.int32 or rs.ndim != 1 or rs.shape != rc.shape:
        raise RuntimeError("lab4d_amd.packed.prune: ray_start / ray_count must be int32 (R,)")
    if rays.deltas.shape[0] != P or rays.xyz.shape[0] != P or rays.dirs.shape[0] != P:
        raise RuntimeError("lab4d_amd.packed.prune: t, deltas, xyz and dirs disagree on the number of rows")
    dev = density.device
    density = density.detach().reshape(P)
    keep = torch.zeros(P, dtype=torch.uint8, device=dev)  # (zeros: the rows that no ray owns are not written)
    count = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call("packed_prune_count", density, rays.deltas, rs, rc, R, P, tau_stop, tau_min, keep, count)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count  # (the exclusive scan: at most P < 2^31 survivors)
    out = {"t": torch.empty(cap, device=dev), "deltas": torch.empty(cap, device=dev), "xyz": torch.empty(cap, 3, device=dev),
           "dirs": torch.empty(cap, 3, device=dev), "ray_idx": torch.empty(cap, dtype=torch.int32, device=dev),
           "src_row": torch.empty(cap, dtype=torch.int32, device=dev), "ray_count": torch.empty(R, dtype=torch.int32, device=dev),
           "total": torch.empty(1, dtype=torch.int32, device=dev)}
    overflow = torch.empty(1, dtype=torch.uint8, device=dev)
    _lib.call("packed_prune_write", keep, rs, rc, start, R, P, cap, aabb, rays.t, rays.deltas, rays.xyz, rays.dirs, out["t"], out["deltas"], out["xyz"],
              out["dirs"], out["ray_idx"], out["src_row"], out["ray_count"], out["total"], overflow)
    return PrunedRays(ray_start=start, overflow=overflow.view(torch.bool), R=R, cap=cap, **out)


# ---------------------------------------------------------------------------------------------------
# distortion loss (include/lab4d_distort.h, csrc/distort.hip)
# ---------------------------------------------------------------------------------------------------
class _PackedDistortion(Function):
    @staticmethod
    def forward(ctx, density, deltas, mid, width, ray_start, ray_count):
        P, R = density.shape[0], ray_start.shape[0]
        loss = torch.empty(R, device=density.device)
        _lib.call("packed_distortion_forward", density, deltas, mid, width, ray_start, ray_count, R, P, loss)
        ctx.save_for_backward(density, deltas, mid, width, ray_start, ray_count)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss):
        density, deltas, mid, width, ray_start, ray_count = ctx.saved_tensors
        P, R = density.shape[0], ray_start.shape[0]
        g_density = torch.zeros_like(density) if ctx.needs_input_grad[0] else None  # (zeros: the rows that no ray owns are not written)
        g_deltas = torch.zeros_like(deltas) if ctx.needs_input_grad[1] else None
        _lib.call("packed_distortion_backward", density, deltas, mid, width, ray_start, ray_count, R, P, g_loss.contiguous(), g_density, g_deltas)
        return g_density, g_deltas, None, None, None, None


def distortion(density, deltas, mid, width, rays):
    """The distortion loss of Barron et al. 2022 (mip-NeRF 360) per ray of a packed list (rules: include/lab4d_distort.h):
    sum_i sum_j w_i w_j |mid_i - mid_j| + (1/3) sum_i w_i^2 width_i with the weights w that `composite` forms from the same density and
    deltas.  density, deltas, mid, width: float32 (P,) or (P,1) on the packed rows of `rays` (a PackedRays, or anything with ray_start /
    ray_count (R,) int32); mid is a row's interval midpoint, ascending within a ray, width >= 0 its width in the units of mid.  -> (R,); a
    ray without samples gives 0.  Differentiable (once) in density and deltas; mid and width are detached."""
    rs, rc = rays.ray_start, rays.ray_count
    _lib.require_device(density, deltas, mid, width, rs, rc)
    P = density.shape[0]
    for name, x in (("density", density), ("deltas", deltas), ("mid", mid), ("width", width)):
        if x.numel() != P or x.dtype != torch.float32 or x.ndim not in (1, 2):
            raise RuntimeError("lab4d_amd.packed.distortion: %s must be float32 (%d,) or (%d, 1), got %s %s" % (name, P, P, x.dtype, tuple(x.shape)))
    if rs.dtype != torch.int32 or rc.dtype != torch.int32 or rs.ndim != 1 or rs.shape != rc.shape:
        raise RuntimeError("lab4d_amd.packed.distortion: ray_start / ray_count must be int32 (R,)")
    return _PackedDistortion.apply(density.reshape(P), deltas.reshape(P), mid.detach().reshape(P), width.detach().reshape(P), rs, rc)


# ---------------------------------------------------------------------------------------------------
# merge of two packed lists per ray by depth (include/lab4d_pmerge.h, csrc/pmerge.hip)
# ---------------------------------------------------------------------------------------------------
class MergedRays:
    """The packed list of one merge: per row (cap rows) t, deltas (copied bit for bit from the source row), ray_idx int32, src int32 = the
    source row in the concatenation [A | B] (i for A's row i, Pa + i for B's row i; -1 in the parked rows).  pos_a (Pa,), pos_b (Pb,) int32:
    the merged row every input row went to, -1 for a row that no ray owns or that fell behind the capacity.  Per ray (R): ray_start,
    ray_count int32 as in a PackedRays; total, overflow likewise.  No xyz / dirs: the two lists may live in different frames."""
    __slots__ = ("t", "deltas", "ray_idx", "src", "pos_a", "pos_b", "ray_start", "ray_count", "total", "overflow", "R", "cap", "Pa", "Pb")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])

    @property
    def from_b(self):
        """(cap,) bool: the row came from list B (False in the parked rows)"""
        return self.src >= self.Pa


def _merge_list(name, rays):
    t, deltas, rs, rc = rays.t, rays.deltas, rays.ray_start, rays.ray_count
    for k, x in (("t", t), ("deltas", deltas)):
        if x.dtype != torch.float32 or x.ndim != 1:
            raise RuntimeError("lab4d_amd.packed.merge: %s.%s must be float32 (n), got %s %s" % (name, k, x.dtype, tuple(x.shape)))
    if deltas.shape[0] != t.shape[0]:
        raise RuntimeError("lab4d_amd.packed.merge: %s.t and %s.deltas disagree on the number of rows" % (name, name))
    if rs.dtype != torch.int32 or rc.dtype != torch.int32 or rs.ndim != 1 or rs.shape != rc.shape:
        raise RuntimeError("lab4d_amd.packed.merge: %s.ray_start / ray_count must be int32 (R,)" % name)
    return t, deltas, rs, rc


@torch.no_grad()
def merge(rays_a, rays_b, cap=None):
    """rays_a, rays_b: two packed lists of the SAME rays -- anything with t, deltas, ray_start, ray_count (a PackedRays, a PrunedRays, a
    MergedRays: three fields merge by merging twice) -- each non-decreasing in t within every ray, as march and prune emit them, with t in
    the same units along the same ray (the lists may have been marched in different frames).  -> MergedRays with `cap` rows (default: the
    rows of both lists, rays_a.cap + rays_b.cap, so that nothing can overflow): per ray the stable z-sort of the concatenation, a tie
    between the lists going to A (rules: include/lab4d_pmerge.h; what MultiFields.compose_fields does on the dense layout).  Two calls
    (count, write) around one prefix sum; no read-back."""
    t_a, d_a, rs_a, rc_a = _merge_list("rays_a", rays_a)
    t_b, d_b, rs_b, rc_b = _merge_list("rays_b", rays_b)
    if rs_a.shape != rs_b.shape:
        raise RuntimeError("lab4d_amd.packed.merge: the lists disagree on the number of rays: %d and %d" % (rs_a.shape[0], rs_b.shape[0]))
    Pa, Pb, R = t_a.shape[0], t_b.shape[0], rs_a.shape[0]
    if Pa + Pb >= 1 << 31:
        raise RuntimeError("lab4d_amd.packed.merge: Pa + Pb = %d + %d does not fit 31 bits" % (Pa, Pb))
    cap = Pa + Pb if cap is None else int(cap)
    if not 0 <= cap < 1 << 31:
        raise RuntimeError("lab4d_amd.packed.merge: cap = %d outside [0, 2^31)" % cap)
    _lib.require_device(t_a, d_a, rs_a, rc_a, t_b, d_b, rs_b, rc_b)
    dev = t_a.device
    count = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call("packed_merge_count", rs_a, rc_a, Pa, rs_b, rc_b, Pb, R, count)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count  # (the exclusive scan: at most Pa + Pb < 2^31 rows)
    out = {"t": torch.empty(cap, device=dev), "deltas": torch.empty(cap, device=dev), "ray_idx": torch.empty(cap, dtype=torch.int32, device=dev),
           "src": torch.empty(cap, dtype=torch.int32, device=dev), "pos_a": torch.empty(Pa, dtype=torch.int32, device=dev),
           "pos_b": torch.empty(Pb, dtype=torch.int32, device=dev), "ray_count": torch.empty(R, dtype=torch.int32, device=dev),
           "total": torch.empty(1, dtype=torch.int32, device=dev)}
    overflow = torch.empty(1, dtype=torch.uint8, device=dev)
    _lib.call("packed_merge_write", t_a.detach(), d_a.detach(), rs_a, rc_a, Pa, t_b.detach(), d_b.detach(), rs_b, rc_b, Pb, R, start, cap, out["t"], out["deltas"],
              out["ray_idx"], out["src"], out["pos_a"], out["pos_b"], out["ray_count"], out["total"], overflow)
    return MergedRays(ray_start=start, overflow=overflow.view(torch.bool), R=R, cap=cap, Pa=Pa, Pb=Pb, **out)


class _MergeRows(Function):
    @staticmethod
    def forward(ctx, a, b, src, pos_a, pos_b, C):
        cap, Pa, Pb = src.shape[0], pos_a.shape[0], pos_b.shape[0]
        out = torch.empty(cap, C, device=src.device)
        _lib.call("packed_merge_gather", a, Pa, b, Pb, src, cap, C, out)
        ctx.save_for_backward(pos_a, pos_b)
        ctx.C = C
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        pos_a, pos_b = ctx.saved_tensors
        g_out, grads = g_out.contiguous(), []
        for need, pos in zip(ctx.needs_input_grad[:2], (pos_a, pos_b)):  # the adjoint of a part: the same gather, through the inverse
            g = torch.empty(pos.shape[0], ctx.C, device=g_out.device) if need else None
            if need:
                _lib.call("packed_merge_gather", g_out, g_out.shape[0], None, 0, pos, pos.shape[0], ctx.C, g)
            grads.append(g)
        return (*grads, None, None, None, None)


def merge_rows(merged, a=None, b=None):
    """Per-row values of the two merged lists in the merged order: a float32 (Pa,) or (Pa, C), b float32 (Pb,) or (Pb, C), 1 <= C <= 64;
    None stands for a block of zeros (a key that only one field produces), both None is an error.  -> (cap,) or (cap, C): row j holds
    a[src[j]], b[src[j] - Pa], or zeros in a parked row.  Differentiable in a and b: the adjoint is the same gather through pos_a / pos_b
    (every value is a copy, so it is the exact transpose)."""
    if a is None and b is None:
        raise RuntimeError("lab4d_amd.packed.merge_rows: a and b are both None")
    ref = a if a is not None else b
    for name, x, n in (("a", a, merged.Pa), ("b", b, merged.Pb)):
        if x is not None and (x.dtype != torch.float32 or x.ndim not in (1, 2) or x.shape[0] != n or x.shape[1:] != ref.shape[1:]):
            raise RuntimeError("lab4d_amd.packed.merge_rows: %s must be float32 (%d,) or (%d, 1..64) with the channels of the other part, got %s %s"
                               % (name, n, n, x.dtype, tuple(x.shape)))
    C = 1 if ref.ndim == 1 else ref.shape[1]
    if not 1 <= C <= 64:
        raise RuntimeError("lab4d_amd.packed.merge_rows: %d channels outside [1, 64]" % C)
    _lib.require_device(a, b, merged.src, merged.pos_a, merged.pos_b)
    out = _MergeRows.apply(None if a is None else a.reshape(-1, C), None if b is None else b.reshape(-1, C), merged.src, merged.pos_a, merged.pos_b, C)
    return out[:, 0] if ref.ndim == 1 else out


# ---------------------------------------------------------------------------------------------------
# importance resampling of a packed list per ray (include/lab4d_presample.h, csrc/presample.hip)
# ---------------------------------------------------------------------------------------------------
def _ray_table(where, rays):
    rs, rc = rays.ray_start, rays.ray_count
    if rs.dtype != torch.int32 or rc.dtype != torch.int32 or rs.ndim != 1 or rs.shape != rc.shape:
        raise RuntimeError("lab4d_amd.packed.%s: ray_start / ray_count must be int32 (R,)" % where)
    return rs, rc


@torch.no_grad()
def weights(density, deltas, rays, with_trans=False):
    """The compositing weights of a packed list, the reference's compute_weights (utils/render_utils.py:99-131) per ray of its own length:
    density, deltas float32 (P,) or (P,1) on the rows of `rays` (a PackedRays, PrunedRays or MergedRays, or anything with ray_start /
    ray_count (R,) int32) -> w (P,): w_i = (1 - exp(-tau_i)) exp(-sum of tau before row i), tau = density * deltas with NaN or a value not
    > 0 counting as 0 (rules: include/lab4d_presample.h); zeros in the rows that no ray owns.  with_trans=True: -> (w, trans (R,)), the
    transmittance behind a ray's last row, 1 for a ray without rows.  No gradients: what `resample` places its rows by."""
    rs, rc = _ray_table("weights", rays)
    P, R = density.shape[0], rs.shape[0]
    for name, x in (("density", density), ("deltas", deltas)):
        if x.numel() != P or x.dtype != torch.float32 or x.ndim not in (1, 2):
            raise RuntimeError("lab4d_amd.packed.weights: %s must be float32 (%d,) or (%d, 1), got %s %s" % (name, P, P, x.dtype, tuple(x.shape)))
    if not (P < 1 << 31 and R < 1 << 31):
        raise RuntimeError("lab4d_amd.packed.weights: P = %d or R = %d does not fit 31 bits" % (P, R))
    _lib.require_device(density, deltas, rs, rc)
    w = torch.zeros(P, device=density.device)  # (zeros: the rows that no ray owns are not written)
    trans = torch.empty(R, device=density.device) if with_trans else None
    _lib.call("packed_weights", density.detach().reshape(P), deltas.detach().reshape(P), rs, rc, R, P, w, trans)
    return (w, trans) if with_trans else w


@torch.no_grad()
def resample(rays, weights, origin, dir, n_imp, *, aabb, u=None, eps=1e-5, cap=None):
    """Inverse-CDF resampling of a packed list into n_imp rows per ray, the reference's importance sampling (nnutils/nerf.py:686-738 with
    render_utils.sample_pdf) for rays of their own lengths.  rays: a PackedRays, a PrunedRays or a MergedRays (t, deltas, ray_start,
    ray_count); weights float32 (P,) or (P,1) on its rows (`weights` above; detached: the placement is not differentiable); origin, dir
    (R,3), the rays the list was marched along; aabb: the box (2,3) / (6,) float32 of the park point (grid.aabb); u: None for the stratified
    centres (k + 0.5) / n_imp, or float32 (R, n_imp) in [0, 1], non-decreasing per ray; eps >= 0 is added to every weight, as sample_pdf
    adds it.  A row of mass m_i = max(w_i, 0) + eps is an interval deltas_i / |dir| wide around t_i that carries m_i evenly; sample k lies
    where the ray's cumulative mass reaches u_k of its total, deltas = the length that carries 1 / n_imp of the mass, at most the source
    row's own (rules: include/lab4d_presample.h).  A ray without rows or without mass emits nothing, every other ray n_imp rows in
    ascending t.  -> PrunedRays with `cap` rows (default R * n_imp: it cannot overflow), src_row = the source row of every new row.  Two
    calls (count, write) around one prefix sum; no read-back."""
    t, deltas = rays.t, rays.deltas
    rs, rc = _ray_table("resample", rays)
    for name, x, tail in (("rays.t", t, ()), ("rays.deltas", deltas, ()), ("origin", origin, (3,)), ("dir", dir, (3,))):
        if x.dtype != torch.float32 or x.ndim != len(tail) + 1 or tuple(x.shape[1:]) != tail:
            raise RuntimeError("lab4d_amd.packed.resample: %s must be float32 (n%s), got %s %s" % (name, "".join(", %d" % c for c in tail), x.dtype, tuple(x.shape)))
    P, R, n_imp, eps = t.shape[0], rs.shape[0], int(n_imp), float(eps)
    if deltas.shape[0] != P:
        raise RuntimeError("lab4d_amd.packed.resample: rays.t and rays.deltas disagree on the number of rows")
    if weights.numel() != P or weights.dtype != torch.float32 or weights.ndim not in (1, 2):
        raise RuntimeError("lab4d_amd.packed.resample: weights must be float32 (%d,) or (%d, 1), got %s %s" % (P, P, weights.dtype, tuple(weights.shape)))
    if origin.shape[0] != R or dir.shape[0] != R:
        raise RuntimeError("lab4d_amd.packed.resample: origin %s and dir %s disagree with the list's %d rays" % (tuple(origin.shape), tuple(dir.shape), R))
    if aabb.numel() != 6 or aabb.dtype != torch.float32:
        raise RuntimeError("lab4d_amd.packed.resample: aabb must be float32 (2, 3) or (6,), got %s %s" % (aabb.dtype, tuple(aabb.shape)))
    if n_imp < 1:
        raise RuntimeError("lab4d_amd.packed.resample: n_imp = %d must be >= 1" % n_imp)
    if not (P < 1 << 31 and R * n_imp < 1 << 31):
        raise RuntimeError("lab4d_amd.packed.resample: P = %d or R * n_imp = %d * %d does not fit 31 bits" % (P, R, n_imp))
    if not (math.isfinite(eps) and eps >= 0):
        raise RuntimeError("lab4d_amd.packed.resample: eps = %r must be finite and >= 0" % eps)
    if u is not None and (u.dtype != torch.float32 or tuple(u.shape) != (R, n_imp)):
        raise RuntimeError("lab4d_amd.packed.resample: u must be float32 (%d, %d), got %s %s" % (R, n_imp, u.dtype, tuple(u.shape)))
    cap = R * n_imp if cap is None else int(cap)
    if not 0 <= cap < 1 << 31:
        raise RuntimeError("lab4d_amd.packed.resample: cap = %d outside [0, 2^31)" % cap)
    _lib.require_device(t, deltas, rs, rc, weights, origin, dir, aabb, u)
    dev = t.device
    weights, t, deltas, origin, dir = weights.detach().reshape(P), t.detach(), deltas.detach(), origin.detach(), dir.detach()
    cdf = torch.zeros(P, device=dev)  # (zeros: the rows that no ray owns are not written)
    mass = torch.empty(R, device=dev)
    count = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call("packed_resample_count", weights, rs, rc, R, P, n_imp, eps, cdf, mass, count)
    start = torch.cumsum(count, 0, dtype=torch.int32) - count  # (the exclusive scan: at most R * n_imp < 2^31 rows)
    out = {"t": torch.empty(cap, device=dev), "deltas": torch.empty(cap, device=dev), "xyz": torch.empty(cap, 3, device=dev),
           "dirs": torch.empty(cap, 3, device=dev), "ray_idx": torch.empty(cap, dtype=torch.int32, device=dev),
           "src_row": torch.empty(cap, dtype=torch.int32, device=dev), "ray_count": torch.empty(R, dtype=torch.int32, device=dev),
           "total": torch.empty(1, dtype=torch.int32, device=dev)}
    overflow = torch.empty(1, dtype=torch.uint8, device=dev)
    _lib.call("packed_resample_write", weights, cdf, mass, t, deltas, rs, rc, start, R, P, origin, dir, None if u is None else u.detach(), n_imp, eps, cap, aabb,
              out["t"], out["deltas"], out["xyz"], out["dirs"], out["ray_idx"], out["src_row"], out["ray_count"], out["total"], overflow)
    return PrunedRays(ray_start=start, overflow=overflow.view(torch.bool), R=R, cap=cap, **out)


# ---------------------------------------------------------------------------------------------------
# proposal loss between two packed lists, and differentiable weights (include/lab4d_proposal.h, csrc/proposal.hip)
# ---------------------------------------------------------------------------------------------------
_RayTable = collections.namedtuple("_RayTable", "ray_start ray_count")


class _RenderWeights(Function):
    @staticmethod
    def forward(ctx, density, deltas, ray_start, ray_count):
        w, trans = weights(density, deltas, _RayTable(ray_start, ray_count), with_trans=True)  # (the forward IS `weights`: one launch site)
        ctx.save_for_backward(density, deltas, ray_start, ray_count)
        return w, trans

    @staticmethod
    @once_differentiable
    def backward(ctx, g_w, g_trans):
        density, deltas, ray_start, ray_count = ctx.saved_tensors
        P, R = density.shape[0], ray_start.shape[0]
        g_density = torch.zeros_like(density)
        _lib.call("packed_weights_backward", density, deltas, ray_start, ray_count, R, P, g_w.contiguous(), g_trans.contiguous(), g_density)
        return g_density, None, None, None


def render_weights(density, deltas, rays, with_trans=False):
    """`weights` with a backward: the compositing weights w (P,) of a packed list (and trans (R,) with with_trans=True), differentiable
    (once) in density -- what a proposal field is trained through (`proposal_loss`).  density, deltas float32 (P,) or (P,1) on the rows of
    `rays`; deltas is detached.  The adjoint recomputes tau, E and w (rules: include/lab4d_proposal.h, WEIGHTS ADJOINT); a row whose tau
    counted as 0 gets no gradient.  `weights` stays the call for a pass without gradients."""
    rs, rc = _ray_table("render_weights", rays)
    P, R = density.shape[0], rs.shape[0]
    for name, x in (("density", density), ("deltas", deltas)):
        if x.numel() != P or x.dtype != torch.float32 or x.ndim not in (1, 2):
            raise RuntimeError("lab4d_amd.packed.render_weights: %s must be float32 (%d,) or (%d, 1), got %s %s" % (name, P, P, x.dtype, tuple(x.shape)))
    if not (P < 1 << 31 and R < 1 << 31):
        raise RuntimeError("lab4d_amd.packed.render_weights: P = %d or R = %d does not fit 31 bits" % (P, R))
    _lib.require_device(density, deltas, rs, rc)
    w, trans = _RenderWeights.apply(density.reshape(P), deltas.detach().reshape(P), rs, rc)
    return (w, trans) if with_trans else w


class _ProposalLoss(Function):
    @staticmethod
    def forward(ctx, w_e, t_e, deltas_e, rs_e, rc_e, w_f, t_f, deltas_f, rs_f, rc_f, dir, eps):
        Pe, Pf, R, dev = w_e.shape[0], w_f.shape[0], rs_e.shape[0], w_e.device
        lo, hi, cdf = torch.zeros(Pe, device=dev), torch.zeros(Pe, device=dev), torch.zeros(Pe, device=dev)  # (zeros: the rows of no ray are not written)
        _lib.call("packed_envelope", w_e, t_e, deltas_e, rs_e, rc_e, dir, R, Pe, lo, hi, cdf)
        span, coef = torch.zeros(Pf, 2, dtype=torch.int32, device=dev), torch.zeros(Pf, device=dev)
        loss = torch.zeros(R, device=dev)
        _lib.call("packed_proposal_forward", lo, hi, cdf, rs_e, rc_e, Pe, w_f, t_f, deltas_f, rs_f, rc_f, Pf, dir, R, eps, span, coef, loss)
        ctx.save_for_backward(span, coef, w_e, rs_e, rc_e, rs_f, rc_f)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss):
        span, coef, w_e, rs_e, rc_e, rs_f, rc_f = ctx.saved_tensors
        g_w_e = torch.zeros_like(w_e)
        _lib.call("packed_proposal_backward", g_loss.contiguous(), span, coef, w_e, rs_e, rc_e, w_e.shape[0], rs_f, rc_f, coef.shape[0], rs_e.shape[0], g_w_e)
        return (g_w_e,) + (None,) * 11


def proposal_loss(rays_env, w_env, rays_fine, w_fine, dir, eps=torch.finfo(torch.float32).eps):
    """The proposal (interval) loss of Barron et al. 2022 (mip-NeRF 360, equation 13) per ray between two packed lists of the SAME rays
    (rules: include/lab4d_proposal.h).  rays_env: the proposal's list (t, deltas, ray_start, ray_count: a PackedRays or a PrunedRays, lo and
    hi non-decreasing per ray as march and prune emit them) with weights w_env float32 (Pe,) or (Pe,1); rays_fine: the fine list (any
    order of intervals, e.g. a resampled list) with weights w_fine (Pf,) or (Pf,1); dir (R,3) the rays both were marched along.  A row is
    the interval deltas / |dir| wide around t.  B_i = the summed weight of the envelope rows that overlap fine row i;
    loss[r] = sum_i max(w_fine_i - B_i, 0)^2 / (w_fine_i + eps).  -> (R,), 0 for a ray without fine rows.  Differentiable (once) in w_env
    only: w_fine is detached, as mip-NeRF 360 stops it.  Three calls (envelope, forward; backward); no read-back, no atomics."""
    eps = float(eps)
    lists = []
    for name, rays, w in (("rays_env", rays_env, w_env), ("rays_fine", rays_fine, w_fine)):
        t, deltas = rays.t, rays.deltas
        rs, rc = _ray_table("proposal_loss", rays)
        for k, x in ((name + ".t", t), (name + ".deltas", deltas)):
            if x.dtype != torch.float32 or x.ndim != 1:
                raise RuntimeError("lab4d_amd.packed.proposal_loss: %s must be float32 (n), got %s %s" % (k, x.dtype, tuple(x.shape)))
        P = t.shape[0]
        if deltas.shape[0] != P:
            raise RuntimeError("lab4d_amd.packed.proposal_loss: %s.t and %s.deltas disagree on the number of rows" % (name, name))
        wname = "w_env" if name == "rays_env" else "w_fine"
        if w.numel() != P or w.dtype != torch.float32 or w.ndim not in (1, 2):
            raise RuntimeError("lab4d_amd.packed.proposal_loss: %s must be float32 (%d,) or (%d, 1), got %s %s" % (wname, P, P, w.dtype, tuple(w.shape)))
        lists.append((w, t, deltas, rs, rc, P))
    (w_e, t_e, d_e, rs_e, rc_e, Pe), (w_f, t_f, d_f, rs_f, rc_f, Pf) = lists
    R = rs_e.shape[0]
    if rs_f.shape[0] != R:
        raise RuntimeError("lab4d_amd.packed.proposal_loss: the lists disagree on the number of rays: %d and %d" % (R, rs_f.shape[0]))
    if dir.dtype != torch.float32 or dir.ndim != 2 or dir.shape[1] != 3:
        raise RuntimeError("lab4d_amd.packed.proposal_loss: dir must be float32 (n, 3), got %s %s" % (dir.dtype, tuple(dir.shape)))
    if dir.shape[0] != R:
        raise RuntimeError("lab4d_amd.packed.proposal_loss: dir %s disagrees with the lists' %d rays" % (tuple(dir.shape), R))
    if not (Pe < 1 << 31 and Pf < 1 << 31 and R < 1 << 31):
        raise RuntimeError("lab4d_amd.packed.proposal_loss: Pe = %d, Pf = %d or R = %d does not fit 31 bits" % (Pe, Pf, R))
    if not (math.isfinite(eps) and eps >= 0):
        raise RuntimeError("lab4d_amd.packed.proposal_loss: eps = %r must be finite and >= 0" % eps)
    _lib.require_device(w_e, t_e, d_e, rs_e, rc_e, w_f, t_f, d_f, rs_f, rc_f, dir)
    return _ProposalLoss.apply(w_e.reshape(Pe), t_e.detach(), d_e.detach(), rs_e, rc_e, w_f.detach().reshape(Pf), t_f.detach(), d_f.detach(), rs_f, rc_f,
                               dir.detach(), eps)
