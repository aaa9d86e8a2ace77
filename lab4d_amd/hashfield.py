"""A field on the multiresolution hash encoding (BASELINE config 5, "hash-grid (instant-NGP) encoding variant").

The reference has NO such field (lab4d/nnutils/nerf.py:98 is a TODO), so this mirrors no reference interface and its
parity against the reference is UNPINNED by nature; the definition follows Mueller et al. 2022 (sections 3 and 5.4) and is checked
against the independent restatement in oracle/hashgrid_oracle.py.  It is shaped like `NeRF.forward(xyz, dir, ..., get_density)`
(nnutils/nerf.py:167-215) so that it can stand where the positional-encoding field stands:
    x in aabb -> [0,1]^3 -> hash_encode (L levels x F features)        csrc/hashgrid.hip        (x outside the box: density = colour = 0)
      -> geometry net  L*F -> 64 -> 16: sdf = out[0], 15 geometry features     LAB4D_NET_HASH_GEO   (the fused chain kernels)
      -> density = VolSDF(sdf)                                                   csrc/flow.hip (as for the posenc field)
      -> colour net  [16 | view direction] -> 64 -> 64 -> 3, sigmoid            LAB4D_NET_HASH_COLOR
Parameters live in a flat dict like every other net here: "hash.table" (L, 2^log2_T, F), "hash.geo.{0,2}.{weight,bias}",
"hash.color.{0,2,4}.{weight,bias}", "logibeta".

Empty-space skipping: an occgrid.OccupancyGrid (a bit per cell of a coarse grid over the box; include/lab4d_occgrid.h) is refreshed from the
field's density with update_occupancy() and handed to forward_compacted(occ=...), whose compaction then also drops the samples in empty cells;
grid.ray_depths() places a ray's samples between its first and last occupied cell.  render_packed() goes all the way: the rays are marched at a
fixed step through the occupied cells only (packed.march), the field runs on the packed list of kept samples, and the list is composited per ray
(packed.composite); nothing of size rays x samples-per-ray exists.  render_packed_pruned() also drops the rows BEHIND the surface before the
differentiable field runs: density() of the kept rows without gradients, packed.prune by transmittance and opacity, forward() on the survivors
(include/lab4d_prune.h).  with_distortion=True on either adds the distortion loss of the list per ray (include/lab4d_distort.h).
render_packed_pair() composites TWO hash fields, an object in front of a scene, into one image: each is marched through its own grid and the two
packed lists are z-merged per ray (include/lab4d_pmerge.h).  render_packed_resampled() renders coarse-to-fine: a march at a coarse step, the
weights of that list without gradients, and the differentiable field on n_imp rows per ray resampled by inverse CDF where the weights are
(include/lab4d_presample.h).  render_packed_proposal() takes those weights from a second, cheaper hash field instead and returns the interval loss
that trains it (include/lab4d_proposal.h).  render_packed_cone() is render_packed() for a scene box many times as wide as the object: the step
grows with the distance and every sample is looked up in a cascade of occupancy grids (occgrid.OccupancyCascade, refreshed with
update_occupancy_cascade(); include/lab4d_conemarch.h).  render_packed(footprint=...) and render_packed_cone(footprint=...) anti-alias the far
field: every row is a Gaussian of radius sample_radius() and reads the encoding's levels footprint-weighted (forward(radius=...);
include/lab4d_hashgrid.h).  All of it is opt-in.

The SDF as an SDF: sdf_gradient() returns the sdf with its gradient in the point from one fused kernel (hashsdf.py, include/lab4d_hashsdf.h),
differentiable in the table and the geometry net; eikonal_loss() and normals() build on it (the counterparts of nnutils/nerf.py:416-493), and
render_packed(with_normal=True) composites a normal map.  Opt-in as well.

The surface without volume rendering: trace_surface() sphere-traces the SDF to one hit per ray (hashtrace.py, include/lab4d_hashtrace.h), and
render_surface() evaluates colour and normal once per ray at that hit -- a preview / eval path, a depth or normal map without a mesh, surface
points for eikonal_loss() and normals().  Opt-in as well.
"""
import collections
import math

import torch
import torch.nn.functional as F

from . import hashgrid, hashsdf, hashtrace, mlp, occgrid, packed
from . import render_utils as RU
from .deformable import volsdf_density

DEFAULT = {"L": 16, "F": 2, "log2_T": 19, "n_min": 16, "n_max": 2048}


def make_weights(seed=0, cfg=None, sdf_bias=None):
    """Random-init parameters of the hash field (tables U(-1e-4, 1e-4) as in the paper, Linear layers Kaiming-uniform like nn.Linear)."""
    c = dict(DEFAULT, **(cfg or {}))
    g = torch.Generator().manual_seed(seed + 977)
    P = {"hash.table": (torch.rand(c["L"], 1 << c["log2_T"], c["F"], generator=g) * 2 - 1) * 1e-4}
    for name, o, i in [("hash.geo.0", 64, c["L"] * c["F"]), ("hash.geo.2", 16, 64), ("hash.color.0", 64, 19), ("hash.color.2", 64, 64), ("hash.color.4", 3, 64)]:
        b = 1.0 / math.sqrt(i)
        P[name + ".weight"] = (torch.rand(o, i, generator=g) * 2 - 1) * b
        P[name + ".bias"] = (torch.rand(o, generator=g) * 2 - 1) * b
    if sdf_bias is not None:
        P["hash.geo.2.bias"][0] = float(sdf_bias)
    P["logibeta"] = torch.tensor([-math.log(0.1)])
    P["aabb"] = torch.tensor([[-0.12, -0.12, -0.12], [0.12, 0.12, 0.12]])
    return P, c


def resolutions(cfg, device):
    return torch.tensor(hashgrid.level_resolutions(cfg["L"], cfg["n_min"], cfg["n_max"]), dtype=torch.int32, device=device)


def _radius01(P, radius):
    """a metric radius in the units of xyz -> the unit cube's: over the SMALLEST edge of P["aabb"], the axis with the smallest cells, so that
    the footprint weights are alias-free on every axis"""
    return (radius.float() / (P["aabb"][1] - P["aabb"][0]).detach().min()).contiguous()


def forward(P, cfg, xyz, dirs, spf, prec=mlp.PREC_F32, res=None, get_density=True, table_grad_f16=False, radius=None, w_min=0.0):
    """xyz, dirs (S,3) -> rgb (S,3), density or sdf (S,1).  spf = samples per frame (the chain kernels' frame stride; the hash nets have
    no per-frame conditioning, any positive value does).
    radius (S,), optional: every sample's isotropic Gaussian radius in the units of xyz (sample_radius() for a marched list); the encoding's
    levels are footprint-weighted (hashgrid.hash_encode(radius=..., w_min=...)): a sample wider than a level's cells reads less of that level,
    and nothing of it below the weight w_min.  0 in a row is a point sample.  No gradient reaches radius.  None: the unweighted encoding."""
    if cfg["L"] * cfg["F"] != 32:
        raise NotImplementedError("hash field: the geometry net is instantiated for L*F = 32 hash features")
    lo, hi = P["aabb"][0], P["aabb"][1]
    x01 = (xyz - lo) / (hi - lo)
    if res is None:
        res = resolutions(cfg, xyz.device)
    f16_from = hashgrid.first_hashed_level(hashgrid.level_resolutions(cfg["L"], cfg["n_min"], cfg["n_max"]), cfg["log2_T"]) if table_grad_f16 else None
    if radius is not None:
        if radius.requires_grad:
            raise RuntimeError("hashfield.forward: radius must not require grad: the footprint weights are not differentiated (pass radius.detach())")
        radius = _radius01(P, radius)
    enc = hashgrid.hash_encode(x01, P["hash.table"], res, cfg["log2_T"], inside_only=True, f16_from=f16_from, radius=radius,
                               w_min=w_min)  # (S, 32); zero rows outside the box (masked below)
    geo = mlp.run_chain(mlp.NET_HASH_GEO, prec, P, enc, spf)                       # (S, 16)
    sdf = geo[:, :1]
    rgb = torch.sigmoid(mlp.run_chain(mlp.NET_HASH_COLOR, prec, P, torch.cat([geo, dirs], -1), spf))
    # The grid is defined on the box (Mueller et al. 2022, section 5.4 / appendix E: rays are marched inside the scene's bounding box only): a sample
    # outside it has no density and no colour.  Its gradient towards the encoding is then exactly zero, and the table-gradient kernel issues no
    # atomic for a zero update (hashgrid_math.hpp: wave_run_add) -- in rounds 1-3 the 89 % of the bench's samples that lie outside the box were
    # clamped onto its boundary cells and their atomics were 68 % of that configuration's step.
    inside = ((x01 >= 0) & (x01 <= 1)).all(-1, keepdim=True).to(rgb.dtype)
    return rgb * inside, ((volsdf_density(sdf, P["logibeta"]) * inside) if get_density else sdf)


def _density_at(P, cfg, pts, prec, chunk):
    """forward()'s density at pts (S,3) in pieces of `chunk` points -> (S,); the view direction does not enter the density"""
    dens = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
    res = resolutions(cfg, pts.device)
    for o in range(0, pts.shape[0], chunk):
        x = pts[o:o + chunk]
        d = torch.zeros_like(x)
        d[:, 2] = 1.0
        dens[o:o + chunk] = forward(P, cfg, x, d, spf=x.shape[0], prec=prec, res=res)[1][:, 0]
    return dens


def _density_where(P, cfg, pts, need, cap, prec, chunk):
    """_density_at on the rows of pts (S,3) whose `need` (S,) bool is set, 0 on the others, in the manner of forward_compacted: the library's
    stream compaction, a gather into `cap` rows (STATIC), the rows behind the count parked outside P["aabb"], a scatter into zeros.
    -> (dens (S,), overflow (1,) bool = more than `cap` rows were needed: the rows behind it got 0).  Nothing is read back."""
    S = pts.shape[0]
    if cap is None or int(cap) < 1:
        raise RuntimeError("hashfield: visible_only=True needs cap, the static number of rows the field is evaluated on (>= 1; a capacity of "
                           "all %d cells would save nothing), got %s" % (S, cap))
    cap = int(cap)
    lo, hi = P["aabb"][0], P["aabb"][1]
    idx, count = RU.compact(need.to(torch.uint8))
    live = (torch.arange(cap, device=pts.device, dtype=torch.int32) < count)[:, None]
    x = torch.where(live, RU.gather_rows_ad(pts, idx, count, cap), (hi + (hi - lo)).to(pts.dtype).expand(cap, 3)).contiguous()
    dens = _density_at(P, cfg, x, prec, chunk)[:, None] * live.to(torch.float32)
    return RU.scatter_rows_ad(dens, idx, count, S)[:, 0].contiguous(), count > cap


@torch.no_grad()
def update_occupancy(P, cfg, grid, prec=mlp.PREC_F32, chunk=1 << 22, visible_only=False, cap=None):
    """Refreshes an occgrid.OccupancyGrid from the field: the density at the grid's cell centres through forward() (in pieces of `chunk`
    points; the view direction does not enter the density), then grid.update -- ema = max(ema * decay, density), bit = ema > thresh.
    Nothing is read back.  Returns the grid.
    visible_only=True (a grid that grid.cull_invisible has culled): the field is evaluated at the centres of the VISIBLE cells only, compacted
    into `cap` rows (a STATIC capacity, required: e.g. int(grid.n_visible) read once after the cull); every other cell gets density 0, which the cull makes of it anyway:
    bits, n_occupied and the ema of the visible cells equal those of the full refresh.  Returns (grid, overflow (1,) bool)."""
    pts = grid.cell_centers()
    if not visible_only:
        return grid.update(_density_at(P, cfg, pts, prec, chunk))
    if grid.visible is None:
        raise RuntimeError("hashfield.update_occupancy: visible_only=True needs a grid culled by cull_invisible")
    dens, overflow = _density_where(P, cfg, pts, occgrid.unpack_bits(grid.visible, grid.G), cap, prec, chunk)
    return grid.update(dens), overflow


def forward_compacted(P, cfg, xyz, dirs, cap, prec=mlp.PREC_F32, res=None, get_density=True, table_grad_f16=False, occ=None, radius=None, w_min=0.0):
    """forward() with the field evaluated on the samples INSIDE the box only (round 6; VERDICT r05 "next" 6): the box mask, the library's stream
    compaction (device-side count, no host round trip: csrc/compact.hip, what the eval path's get_valid_idx uses), a gather of the points / view
    directions into a buffer of `cap` rows, encoding + both nets + the table gradient on that buffer, a scatter of colour / density into zeros.
    A ray marched through the bench's scene spends 11 % of its samples inside the box: everything per-sample behind the ray sampler runs on a ninth
    of the rows.  Same values as forward() on the inside samples (the per-sample arithmetic does not depend on the row a sample sits in), zeros
    outside, gradients to the table, the Linears and the points.  `cap` is a STATIC capacity (the call is captured into hipGraphs); rows behind the
    count are parked outside the box (zero encoding, masked); a count above `cap` would drop samples: the returned `overflow` (device bool) says so,
    callers check it where they synchronise anyway.  Returns (rgb (S,3), density | sdf (S,1), count (1) int32, overflow (1) bool).
    occ: an occgrid.OccupancyGrid over P["aabb"] (optional): the compaction mask becomes occ.mask(xyz) -- inside the box AND in a cell whose bit
    is set -- so samples in empty cells get zero colour and density and cost nothing behind the mask, like the samples outside the box.  A grid that
    has not been updated yet has every bit set and changes nothing.  None: the box test alone, as before.
    radius (S,), w_min: forward()'s; the radius is gathered with the points, the parked rows get radius 0."""
    S = xyz.shape[0]
    if radius is not None and radius.requires_grad:
        raise RuntimeError("hashfield.forward_compacted: radius must not require grad: the footprint weights are not differentiated (pass radius.detach())")
    lo, hi = P["aabb"][0], P["aabb"][1]
    with torch.no_grad():
        if occ is None:
            x01 = (xyz - lo) / (hi - lo)
            mask = ((x01 >= 0) & (x01 <= 1)).all(-1).to(torch.uint8)
        else:
            mask = occ.mask(xyz)  # one kernel: the same x01 and box test, and the bit of the sample's cell
        idx, count = RU.compact(mask)
        live = (torch.arange(cap, device=xyz.device, dtype=torch.int32) < count)[:, None]
        overflow = count > cap
    xyz_c = RU.gather_rows_ad(xyz, idx, count, cap)
    xyz_c = torch.where(live, xyz_c, (hi + (hi - lo)).expand_as(xyz_c))  # rows behind the count: a point outside the box
    dirs_c = RU.gather_rows_ad(dirs, idx, count, cap)
    radius_c = None
    if radius is not None:  # (gathered like the points; the rows behind the count are point samples)
        radius_c = torch.where(live, RU.gather_rows_ad(radius.float().reshape(S, 1), idx, count, cap), torch.zeros((), device=xyz.device))[:, 0].contiguous()
    rgb_c, d_c = forward(P, cfg, xyz_c, dirs_c, spf=cap, prec=prec, res=res, get_density=get_density, table_grad_f16=table_grad_f16, radius=radius_c,
                         w_min=w_min)
    if not get_density:
        d_c = d_c * live.to(d_c.dtype)  # (forward() masks density and colour, not the raw sdf)
    return RU.scatter_rows_ad(rgb_c, idx, count, S), RU.scatter_rows_ad(d_c, idx, count, S), count, overflow


def sdf_gradient(P, cfg, xyz, res=None, work_rows=None):
    """xyz (S,3) in the field's frame (must not require grad) -> sdf (S,1), grad (S,3) = d sdf / d xyz = grad01 / (hi - lo), from ONE fused
    kernel (csrc/hashsdf.hip): the encoding, the geometry net 32 -> 64, ReLU -> row 0 of the head, and the chain rule through both.  What
    compute_gradient(fn, x) gives the positional-encoding fields (utils/torch_utils.py:4-27, nnutils/nerf.py:437).  The derivative is the
    one of the grid cell the point lies in.  Outside the box grad = 0 and sdf is what forward(get_density=False) returns there.  Both
    outputs are differentiable (once) in hash.table, hash.geo.0.* and hash.geo.2.*, whose rows 1..15 get exact zeros; there is no
    gradient to the points.  work_rows: see hashsdf.sdf_grad01."""
    if cfg["L"] * cfg["F"] != 32:
        raise NotImplementedError("hash field: the geometry net is instantiated for L*F = 32 hash features")
    if xyz.requires_grad:
        raise RuntimeError("hashfield.sdf_gradient: xyz must not require grad: second derivatives in the points are not implemented (pass xyz.detach())")
    lo, hi = P["aabb"][0], P["aabb"][1]
    x01 = (xyz - lo) / (hi - lo)
    if res is None:
        res = resolutions(cfg, xyz.device)
    sdf, g01 = hashsdf.sdf_grad01(x01, P["hash.table"], res, cfg["log2_T"], P["hash.geo.0.weight"], P["hash.geo.0.bias"], P["hash.geo.2.weight"][0],
                                  P["hash.geo.2.bias"][:1], work_rows=work_rows)
    return sdf[:, None], g01 / (hi - lo)


def eikonal_loss(P, cfg, xyz, res=None, work_rows=None):
    """(|grad sdf| - 1)^2 per point, (S,1): the form of nnutils/nerf.py:451,486, times the inside mask (a point outside the box has no
    geometry to regularise).  Where grad == 0 the norm's derivative is torch's (zero).  Gradients as in sdf_gradient."""
    lo, hi = P["aabb"][0], P["aabb"][1]
    x01 = (xyz - lo) / (hi - lo)
    inside = ((x01 >= 0) & (x01 <= 1)).all(-1, keepdim=True).to(torch.float32)
    _, grad = sdf_gradient(P, cfg, xyz, res=res, work_rows=work_rows)
    return (grad.norm(2, -1, keepdim=True) - 1) ** 2 * inside


@torch.no_grad()
def normals(P, cfg, xyz, res=None):
    """Unit normals (S,3) in the field's frame: F.normalize(grad sdf); zero where the gradient is zero (outside the box).  No gradients.
    The reference flips the sign of its normals towards the camera (the ECON convention of nnutils/nerf.py:489-491: a multiplication by [1, -1, -1]): that flip belongs to
    camera space, where the view direction is known, and is NOT applied here."""
    return F.normalize(sdf_gradient(P, cfg, xyz.detach(), res=res)[1], dim=-1)


def _packed_distortion(dens_s, rays, dt):
    """The distortion loss (R,1) of a marched or pruned list in metric units, so that it does not depend on the length of `dir`: a row's
    interval is one step, width = rays.deltas = dt |d|, around mid = rays.t * rays.deltas / dt = t |d|."""
    return packed.distortion(dens_s, rays.deltas, rays.t * rays.deltas / dt, rays.deltas, rays)[:, None]


def sample_radius(rays, dir, footprint):
    """The isotropic Gaussian radius (cap,) of every row of a marched list (packed.march / packed.march_cone), in the units of xyz: the pixel
    cone's radius at the sample, rays.t * |dir[ray_idx]| * footprint, where `footprint` is the cone's Gaussian radius per unit of metric
    distance (for a pinhole camera about the pixel's angular width over sqrt(12)).  0 in the parked rows (ray_idx == -1).  No gradients."""
    with torch.no_grad():
        live = rays.ray_idx >= 0
        if dir.shape[0] == 0:  # (no rays: every row is parked)
            return torch.zeros_like(rays.t)
        length = dir.detach().norm(2, -1)[rays.ray_idx.clamp_min(0).long()]
        return torch.where(live, rays.t * length * float(footprint), torch.zeros_like(rays.t)).contiguous()


def _footprint_radius(rays, dir, footprint, with_normal):
    if footprint is None:
        return None
    if with_normal:
        raise NotImplementedError("hashfield: footprint together with with_normal=True: the fused SDF-gradient kernel (csrc/hashsdf.hip) reads the "
                                  "unweighted encoding")
    return sample_radius(rays, dir, footprint)


def render_packed(P, cfg, grid, origin, dir, t_range, dt, cap, prec=mlp.PREC_F32, table_grad_f16=False, k_max=1024, res=None, with_normal=False,
                  with_distortion=False, footprint=None, w_min=1.0 / 256):
    """Renders rays through the hash field with packed marching (include/lab4d_packed.h): packed.march(grid, origin, dir, t_range, dt, cap, k_max)
    keeps the candidates t0 + (k + 0.5) dt of every ray whose cell's bit is set -- what forward_compacted(occ=grid) keeps of the same lattice --
    as one packed list of at most `cap` rows (STATIC: the call is capturable), forward() runs on those rows (the parked rows behind the count lie
    outside the box: zero encoding, masked), and packed.composite renders colour and depth per ray with delta = dt * |dir|.  origin, dir (R,3) in the
    field's frame, t_range (R,2).  Returns (rgb (R,3), mask (R,1), depth (R,1), total (1,) int32 = kept samples before the capacity, overflow (1,) bool =
    total > cap: samples were dropped, callers check it where they synchronise anyway).  A ray without a kept sample renders zeros.  Gradients flow
    to the table, the Linears and logibeta.
    with_normal=True: normals() of the kept rows is composited like the colour and `normal (R,3)` is appended to the returned tuple (the
    weighted mean of unit normals: not renormalised; gradients reach it through the weights only).  The other five are unchanged.
    with_distortion=True: `distortion (R,1)`, packed.distortion of the kept rows in metric units (width = dt |dir|, mid = t |dir|), is appended
    LAST, behind `normal` when both are set; gradients reach the table, the geometry Linears and logibeta through the density.
    footprint: the pixel cone's Gaussian radius per unit of metric distance (optional): forward() gets radius = sample_radius(rays, dir, footprint)
    and w_min, so the far rows read footprint-weighted levels.  Not together with with_normal=True (NotImplementedError)."""
    rays = packed.march(grid, origin, dir, t_range, dt, cap, k_max=k_max)
    rgb_s, dens_s = forward(P, cfg, rays.xyz, rays.dirs, spf=max(int(cap), 1), prec=prec, res=res, table_grad_f16=table_grad_f16,
                            radius=_footprint_radius(rays, dir, footprint, with_normal), w_min=w_min)
    fields = {"rgb": rgb_s, "depth": rays.t[:, None]}
    if with_normal:
        fields["normal"] = normals(P, cfg, rays.xyz, res=res)
    rendered, mask = packed.composite(dens_s, rays.deltas, fields, rays)
    out = (rendered["rgb"], mask, rendered["depth"], rays.total, rays.overflow)
    if with_normal:
        out += (rendered["normal"],)
    return out + (_packed_distortion(dens_s, rays, dt),) if with_distortion else out


@torch.no_grad()
def update_occupancy_cascade(P, cfg, cascade, prec=mlp.PREC_F32, chunk=1 << 22, visible_only=False, cap=None):
    """Refreshes an occgrid.OccupancyCascade from the field: the density at every level's cell centres through forward() (in pieces of
    `chunk` points), then cascade.update -- the propagation from fine to coarse, then ema = max(ema * decay, density), bit = ema > thresh
    per level.  The field lives on the OUTERMOST box, as in the paper: P["aabb"] must equal cascade.aabbs[K - 1], which is checked first
    (the one read-back of this call) and raises otherwise.  Returns the cascade.
    visible_only=True (a cascade that cascade.cull_invisible has culled): the field is evaluated on cascade.refresh_set() only -- the visible
    cells and the cells below a visible cell of a coarser level, whose density the propagation carries into that visible cell -- compacted
    into `cap` rows (a STATIC capacity, required: e.g. int(cascade.refresh_set().sum()) read once after the cull); every other cell gets density 0.  bits, n_occupied and the ema
    of the visible cells equal those of the full refresh.  Returns (cascade, overflow (1,) bool)."""
    outer = cascade.aabbs[cascade.K - 1]
    box = P["aabb"]
    if box.numel() != 6 or not torch.equal(box.detach().reshape(6).to(device=outer.device, dtype=torch.float32), outer):
        raise RuntimeError("hashfield.update_occupancy_cascade: P[\"aabb\"] must be the cascade's outermost box aabbs[K - 1] = %s, got %s"
                           % (outer.tolist(), box.reshape(-1).tolist()))
    pts = cascade.cell_centers().reshape(-1, 3)
    if not visible_only:
        return cascade.update(_density_at(P, cfg, pts, prec, chunk).reshape(cascade.K, -1))
    if cascade.visible is None:
        raise RuntimeError("hashfield.update_occupancy_cascade: visible_only=True needs a cascade culled by cull_invisible")
    dens, overflow = _density_where(P, cfg, pts, cascade.refresh_set().reshape(-1), cap, prec, chunk)
    return cascade.update(dens.reshape(cascade.K, -1)), overflow


def render_packed_cone(P, cfg, cascade, origin, dir, t_range, cone, dt_min, dt_max, cap, prec=mlp.PREC_F32, table_grad_f16=False, k_max=1024, res=None,
                       with_normal=False, with_distortion=False, footprint=None, w_min=1.0 / 256):
    """render_packed() with the cone-stepped march through a cascade of occupancy grids (include/lab4d_conemarch.h), for a scene box many
    times as wide as the object: packed.march_cone(cascade, origin, dir, t_range, cone, dt_min, dt_max, cap, k_max) steps every ray at
    s = clamp(a * cone, dt_min, dt_max) and keeps a candidate iff its bit is set at the cascade level that fits its position and its step;
    forward() runs on the kept rows (P["aabb"] is the cascade's outermost box; the parked rows lie outside it) and packed.composite renders
    them with each row's OWN delta = s |dir|.  Returns what render_packed returns: (rgb (R,3), mask (R,1), depth (R,1), total, overflow), then
    `normal (R,3)` with with_normal=True, then `distortion (R,1)` with with_distortion=True: packed.distortion with mid = t and width = steps
    per row, in the units of t.  Gradients flow to the table, the Linears and logibeta.
    footprint, w_min: as in render_packed -- the anti-aliased far field: a row at distance t reads level l times erf(1 / (sqrt(8) sigma n_l)) with
    sigma = t |dir| footprint over the box's smallest edge, and nothing of the levels whose weight lies below w_min."""
    rays = packed.march_cone(cascade, origin, dir, t_range, cone, dt_min, dt_max, cap, k_max=k_max)
    rgb_s, dens_s = forward(P, cfg, rays.xyz, rays.dirs, spf=max(int(cap), 1), prec=prec, res=res, table_grad_f16=table_grad_f16,
                            radius=_footprint_radius(rays, dir, footprint, with_normal), w_min=w_min)
    fields = {"rgb": rgb_s, "depth": rays.t[:, None]}
    if with_normal:
        fields["normal"] = normals(P, cfg, rays.xyz, res=res)
    rendered, mask = packed.composite(dens_s, rays.deltas, fields, rays)
    out = (rendered["rgb"], mask, rendered["depth"], rays.total, rays.overflow)
    if with_normal:
        out += (rendered["normal"],)
    return out + (packed.distortion(dens_s, rays.deltas, rays.t, rays.steps, rays)[:, None],) if with_distortion else out


def density(P, cfg, xyz, prec=mlp.PREC_F32, res=None):
    """xyz (S,3) -> density (S,1): forward()'s encoding (inside_only), geometry chain and volsdf_density, masked outside the box -- without
    the colour net, for a pass that only asks where a ray becomes opaque (render_packed_pruned).  The per-sample arithmetic is forward()'s
    own: the same rows give, bit for bit, the density forward() returns at the same precision."""
    if cfg["L"] * cfg["F"] != 32:
        raise NotImplementedError("hash field: the geometry net is instantiated for L*F = 32 hash features")
    lo, hi = P["aabb"][0], P["aabb"][1]
    x01 = (xyz - lo) / (hi - lo)
    if res is None:
        res = resolutions(cfg, xyz.device)
    enc = hashgrid.hash_encode(x01, P["hash.table"], res, cfg["log2_T"], inside_only=True)
    geo = mlp.run_chain(mlp.NET_HASH_GEO, prec, P, enc, max(int(xyz.shape[0]), 1))
    inside = ((x01 >= 0) & (x01 <= 1)).all(-1, keepdim=True).to(geo.dtype)
    return volsdf_density(geo[:, :1], P["logibeta"]) * inside


def render_packed_pruned(P, cfg, grid, origin, dir, t_range, dt, cap, prec=mlp.PREC_F32, table_grad_f16=False, k_max=1024, res=None, with_normal=False,
                         early_stop_eps=1e-4, alpha_thre=0.0, prune_cap=None, with_distortion=False):
    """render_packed() with the rows behind the surface dropped before the differentiable field runs (include/lab4d_prune.h), the two-pass form of
    Mueller et al. 2022 and nerfacc: packed.march as in render_packed; density() of the kept rows under no_grad; packed.prune drops every row at
    and behind the point where its ray's transmittance has fallen below early_stop_eps, and every row whose opacity lies below alpha_thre;
    forward() runs on the survivors (at most prune_cap rows, default cap; STATIC like cap) and packed.composite renders them with the pruned
    (start, count).  With alpha_thre = 0 what is dropped of a ray weighs less than early_stop_eps in total.  Returns (rgb, mask, depth, total,
    overflow, kept, kept_overflow): the first five as in render_packed (total / overflow are the march's), kept (1,) int32 = the survivors before
    prune_cap, kept_overflow (1,) bool = kept > prune_cap; `normal` is appended with with_normal=True, and behind it `distortion (R,1)` with
    with_distortion=True: render_packed's, on the pruned list's own rows.  Gradients flow to the table, the Linears and logibeta through the
    surviving rows only: the prune decision itself is not differentiable."""
    rays = packed.march(grid, origin, dir, t_range, dt, cap, k_max=k_max)
    with torch.no_grad():
        dens0 = density(P, cfg, rays.xyz, prec=prec, res=res)
    kept = packed.prune(rays, dens0, early_stop_eps=early_stop_eps, alpha_thre=alpha_thre, cap=prune_cap, aabb=grid.aabb)
    rgb_s, dens_s = forward(P, cfg, kept.xyz, kept.dirs, spf=max(kept.cap, 1), prec=prec, res=res, table_grad_f16=table_grad_f16)
    fields = {"rgb": rgb_s, "depth": kept.t[:, None]}
    if with_normal:
        fields["normal"] = normals(P, cfg, kept.xyz, res=res)
    rendered, mask = packed.composite(dens_s, kept.deltas, fields, kept)
    out = (rendered["rgb"], mask, rendered["depth"], rays.total, rays.overflow, kept.total, kept.overflow)
    if with_normal:
        out += (rendered["normal"],)
    return out + (_packed_distortion(dens_s, kept, dt),) if with_distortion else out


def render_packed_resampled(P, cfg, grid, origin, dir, t_range, dt, cap, n_imp, fine_cap=None, u=None, eps=1e-5, prec=mlp.PREC_F32, table_grad_f16=False,
                            k_max=1024, res=None):
    """render_packed() coarse-to-fine (include/lab4d_presample.h), the reference's importance sampling (nnutils/nerf.py:686-738) on packed
    lists: packed.march at the COARSE step dt; density() of the marched rows under no_grad; packed.weights turns it into the compositing
    weights of the coarse list; packed.resample places n_imp new rows per ray where those weights are (u, eps: see there; at most fine_cap
    rows, default R * n_imp: no overflow; STATIC like cap); forward() runs on the new rows ONLY and packed.composite renders them with
    depth = t.  The sample positions are detached, as the reference detaches them; gradients reach the table, the Linears and logibeta.
    A ray without marched rows, or whose rows weigh nothing with eps = 0, renders zeros.  Returns (rgb (R,3), mask (R,1), depth (R,1),
    total, overflow (the march's), total_fine (1,) int32 = the resampled rows before fine_cap, overflow_fine (1,) bool)."""
    rays = packed.march(grid, origin, dir, t_range, dt, cap, k_max=k_max)
    with torch.no_grad():
        dens0 = density(P, cfg, rays.xyz, prec=prec, res=res)
        fine = packed.resample(rays, packed.weights(dens0, rays.deltas, rays), origin, dir, n_imp, aabb=grid.aabb, u=u, eps=eps, cap=fine_cap)
    rgb_s, dens_s = forward(P, cfg, fine.xyz, fine.dirs, spf=max(fine.cap, 1), prec=prec, res=res, table_grad_f16=table_grad_f16)
    rendered, mask = packed.composite(dens_s, fine.deltas, {"rgb": rgb_s, "depth": fine.t[:, None]}, fine)
    return rendered["rgb"], mask, rendered["depth"], rays.total, rays.overflow, fine.total, fine.overflow


def render_packed_proposal(Pp, cfgp, P, cfg, grid, origin, dir, t_range, dt, cap, n_imp, fine_cap=None, u=None, eps=1e-5, prec=mlp.PREC_F32,
                           table_grad_f16=False, k_max=1024, res=None, resp=None, loss_eps=torch.finfo(torch.float32).eps):
    """render_packed_resampled() with a TRAINED proposal field (include/lab4d_proposal.h), the scheme of Barron et al. 2022 (mip-NeRF 360):
    the coarse pass runs a second, cheaper hash field (Pp, cfgp: a small table) instead of the main one.  packed.march at the step dt;
    density(Pp, cfgp) of the marched rows WITH gradients; packed.render_weights turns it into the weights of the coarse list;
    packed.resample places n_imp rows per ray by the detached weights (u, eps, fine_cap: see render_packed_resampled); forward(P, cfg) runs
    on the new rows and packed.composite renders them; packed.weights of the fine list under no_grad; packed.proposal_loss (loss_eps) holds
    the coarse weights above the fine ones.  Returns render_packed_resampled's tuple with prop_loss (R,1) appended.  The image's gradients
    reach P only (the sample positions are detached), the loss's gradients reach Pp only (the fine weights are detached): one backward of
    image loss + prop_loss.mean() trains both.  res / resp: the level resolutions of cfg / cfgp."""
    rays = packed.march(grid, origin, dir, t_range, dt, cap, k_max=k_max)
    dens_p = density(Pp, cfgp, rays.xyz, prec=prec, res=resp)
    w_p = packed.render_weights(dens_p, rays.deltas, rays)
    fine = packed.resample(rays, w_p.detach(), origin, dir, n_imp, aabb=grid.aabb, u=u, eps=eps, cap=fine_cap)
    rgb_s, dens_s = forward(P, cfg, fine.xyz, fine.dirs, spf=max(fine.cap, 1), prec=prec, res=res, table_grad_f16=table_grad_f16)
    rendered, mask = packed.composite(dens_s, fine.deltas, {"rgb": rgb_s, "depth": fine.t[:, None]}, fine)
    with torch.no_grad():
        w_f = packed.weights(dens_s, fine.deltas, fine)
    prop_loss = packed.proposal_loss(rays, w_p, fine, w_f, dir, eps=loss_eps)[:, None]
    return rendered["rgb"], mask, rendered["depth"], rays.total, rays.overflow, fine.total, fine.overflow, prop_loss


PackedField = collections.namedtuple("PackedField", "P cfg grid origin dir t_range dt cap")
PairRender = collections.namedtuple("PairRender", "rgb mask depth mask_a mask_b total_a overflow_a total_b overflow_b total overflow")


def render_packed_pair(a, b, merged_cap=None, prec=mlp.PREC_F32, table_grad_f16=False, k_max=1024, res_a=None, res_b=None):
    """Two hash fields composited into one image: an object in front of a scene, the "comp" configurations' compose_fields
    (nnutils/multifields.py:339-398) on packed lists (include/lab4d_pmerge.h).  a, b: a PackedField each -- its parameters and cfg, its
    occupancy grid, the SAME R rays as origin, dir (R,3) and t_range (R,2) in the field's OWN frame, its step dt and its STATIC capacity.
    Both must measure t in the same units along a ray (a rigid transform between the frames keeps it; a scale does not).  Each field is
    marched through its own grid (packed.march) and evaluated on its own rows (forward()); packed.merge z-sorts the two lists per ray
    (a tie goes to `a`) into at most merged_cap rows (default a.cap + b.cap: no overflow), packed.merge_rows gathers rgb, the density,
    density_a (b's block zero) and density_b (a's block zero), and packed.composite renders them over the merged (start, count) with
    depth = merged.t.  mask_a / mask_b are the rendered density_a / density_b over (their sum + 1e-6), as utils/render_utils.py:172-183
    turns density_fg / density_bg into mask_fg / mask_bg.  -> PairRender(rgb (R,3), mask, depth, mask_a, mask_b (R,1), total_a,
    overflow_a, total_b, overflow_b (the marches'), total, overflow (the merge's)).  Gradients reach both fields' tables, Linears and
    logibeta."""
    rays_a = packed.march(a.grid, a.origin, a.dir, a.t_range, a.dt, a.cap, k_max=k_max)
    rays_b = packed.march(b.grid, b.origin, b.dir, b.t_range, b.dt, b.cap, k_max=k_max)
    rgb_a, dens_a = forward(a.P, a.cfg, rays_a.xyz, rays_a.dirs, spf=max(int(a.cap), 1), prec=prec, res=res_a, table_grad_f16=table_grad_f16)
    rgb_b, dens_b = forward(b.P, b.cfg, rays_b.xyz, rays_b.dirs, spf=max(int(b.cap), 1), prec=prec, res=res_b, table_grad_f16=table_grad_f16)
    merged = packed.merge(rays_a, rays_b, cap=merged_cap)
    fields = {"rgb": packed.merge_rows(merged, rgb_a, rgb_b), "depth": merged.t[:, None], "density_a": packed.merge_rows(merged, a=dens_a),
              "density_b": packed.merge_rows(merged, b=dens_b)}
    rendered, mask = packed.composite(packed.merge_rows(merged, dens_a, dens_b), merged.deltas, fields, merged)
    density_sum = rendered["density_a"] + rendered["density_b"] + 1e-6
    return PairRender(rendered["rgb"], mask, rendered["depth"], rendered["density_a"] / density_sum, rendered["density_b"] / density_sum, rays_a.total,
                      rays_a.overflow, rays_b.total, rays_b.overflow, merged.total, merged.overflow)


Surface = collections.namedtuple("Surface", "t status n_eval sdf xyz hit")


@torch.no_grad()
def trace_surface(P, cfg, origin, dir, t_range, grid=None, eps=1e-4, step_scale=1.0, min_step=None, max_steps=128, n_bisect=8, res=None):
    """Sphere-traces the field's SDF along the rays origin + t dir, t in t_range (origin, dir (R,3) in the field's frame, dir of any length,
    t_range (R,2)), to one hit per ray (include/lab4d_hashtrace.h; ONE kernel, csrc/hashtrace.hip): steps of max(step_scale * sdf, min_step) / |dir|
    (min_step defaults to eps) until |sdf| <= eps, a bisection of at most n_bisect evaluations where the sign changes, at most max_steps steps.
    Returns Surface(t (R,), status (R,) int32 -- hashtrace.MISS / CONVERGED / BRACKETED / STARTS_INSIDE / OUT_OF_STEPS --, n_eval (R,) int32,
    sdf (R,) at the hit, xyz (R,3) = origin + t dir, hit (R,) bool = status 1, 2 or 3).
    grid: an occgrid.OccupancyGrid over P["aabb"] (optional): grid.ray_span narrows t_range to the ray's first .. last occupied cell first; a
    ray that the span misses is traced with an empty range and gets status MISS with t = its own t0.  No gradients."""
    if cfg["L"] * cfg["F"] != 32:
        raise NotImplementedError("hash field: the geometry net is instantiated for L*F = 32 hash features")
    if res is None:
        res = resolutions(cfg, origin.device)
    if grid is not None:
        span, seen = grid.ray_span(origin, dir, t_range)
        empty = torch.stack([t_range[:, 0], torch.full_like(t_range[:, 0], -math.inf)], -1)  # (t1 is not finite: rejected, t_hit = t0)
        t_range = torch.where(seen[:, None], span, empty).contiguous()
    t, status, n_eval, sdf = hashtrace.trace(origin, dir, t_range, P["aabb"], P["hash.table"], res, cfg["log2_T"], P["hash.geo.0.weight"],
                                             P["hash.geo.0.bias"], P["hash.geo.2.weight"][0], P["hash.geo.2.bias"][:1], eps=eps, step_scale=step_scale,
                                             min_step=min_step, max_steps=max_steps, n_bisect=n_bisect)
    hit = (status >= hashtrace.CONVERGED) & (status <= hashtrace.STARTS_INSIDE)
    return Surface(t, status, n_eval, sdf, origin + t[:, None] * dir, hit)


def render_surface(P, cfg, origin, dir, t_range, grid=None, prec=mlp.PREC_F32, differentiable=False, **trace_kw):
    """Renders the field's SURFACE: trace_surface(P, cfg, origin, dir, t_range, grid, **trace_kw), then one sdf_gradient() and one forward() per
    ray at the hit point with the unit direction.  Returns rgb (R,3), mask (R,1) = hit, depth (R,1) = t of the hit, normal (R,3) =
    F.normalize(grad sdf).  A ray without a hit is parked outside the box (hi + (hi - lo), forward_compacted's rule) and renders zeros.
    differentiable=False: the hit is a constant; rgb and normal are differentiable in the parameters at that fixed point, depth in nothing.
    differentiable=True: depth = t - (sdf - sdf.detach()) / (grad.detach() . dir) -- the derivative of the implicit surface sdf(o + t d) = 0:
    the VALUE is t bit for bit, the gradient reaches the table and the geometry net -- and the colour is evaluated at origin + depth * dir, so
    that it gets a gradient through the point as well.  Rays with |grad . dir| < 1e-6 (grazing) keep the plain t."""
    if "res" not in trace_kw or trace_kw["res"] is None:
        trace_kw["res"] = resolutions(cfg, origin.device)
    res = trace_kw["res"]
    s = trace_surface(P, cfg, origin, dir, t_range, grid=grid, **trace_kw)
    lo, hi = P["aabb"][0].detach(), P["aabb"][1].detach()
    hit = s.hit[:, None]
    park = (hi + (hi - lo)).expand_as(s.xyz)
    unit = F.normalize(dir.detach(), dim=-1)
    x = torch.where(hit, s.xyz, park).contiguous()
    sdf, grad = sdf_gradient(P, cfg, x, res=res)
    depth = s.t[:, None]
    if differentiable:
        gd = (grad.detach() * dir.detach()).sum(-1, keepdim=True)
        ok = hit & (gd.abs() >= 1e-6)
        depth = depth - torch.where(ok, (sdf - sdf.detach()) / torch.where(ok, gd, torch.ones_like(gd)), torch.zeros_like(gd))
        x = torch.where(hit, origin.detach() + depth * dir.detach(), park)
    rgb = forward(P, cfg, x, unit, spf=max(int(x.shape[0]), 1), prec=prec, res=res, get_density=False)[0]  # (zero outside the box: the parked rows)
    mask = hit.to(rgb.dtype)
    # (where, not a product with the mask: a rejected ray's t may be NaN)
    return rgb * mask, mask, torch.where(hit, depth, torch.zeros_like(depth)), F.normalize(grad, dim=-1) * mask
