"""Occupancy bit grid of the hash field (include/lab4d_occgrid.h, csrc/occgrid.hip): a bit per cell of a G^3 grid over the field's box,
refreshed from the field's own density (hashfield.update_occupancy), consulted per sample (`mask`: the compaction mask of
hashfield.forward_compacted) and per ray (`ray_span` / `ray_depths`: march only between the first and the last occupied cell).  The
reference has no counterpart (nnutils/nerf.py:98 is a TODO); the rules are written down in the header and in csrc/occgrid_math.hpp.
Nothing here synchronises with the host: every call can be captured in a hipGraph."""
import torch

from . import _lib


def _f32(name, t, *shape_tail):
    _lib.require_device(t)
    if t.dtype != torch.float32 or t.ndim < 1 or tuple(t.shape[-len(shape_tail):]) != shape_tail:
        raise RuntimeError("lab4d_amd.occgrid: %s must be float32 (..., %s), got %s %s" % (name, ", ".join(map(str, shape_tail)), t.dtype, tuple(t.shape)))


class OccupancyGrid:
    """bits (ceil(G^3/32),) int32 words (bit idx & 31 of word idx >> 5, idx = (i*G + j)*G + k, x slowest), ema (G^3,) fp32, n_occupied (1,)
    device int32.  A new grid knows nothing: every bit is set, ema = +inf, and its mask is the box test alone."""

    def __init__(self, aabb, G=128, decay=0.95, thresh=0.01):
        G = int(G)
        if not 2 <= G <= 256:
            raise RuntimeError("lab4d_amd.occgrid: G = %d outside [2, 256]" % G)
        if not torch.is_tensor(aabb):
            raise RuntimeError("lab4d_amd.occgrid: aabb must be a (2, 3) device tensor")
        _lib.require_device(aabb)
        if tuple(aabb.shape) != (2, 3):
            raise RuntimeError("lab4d_amd.occgrid: aabb must be (2, 3), got %s" % (tuple(aabb.shape),))
        self.G, self.decay, self.thresh = G, float(decay), float(thresh)
        self.aabb = aabb.detach().to(torch.float32).contiguous()  # (a device tensor stays on the device: no host copy of the box)
        dev = self.aabb.device
        n = G ** 3
        self.bits = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device=dev)
        if n % 32:
            self.bits[-1] = (1 << (n % 32)) - 1  # the unused bits of the last word are zero
        self.ema = torch.full((n,), float("inf"), dtype=torch.float32, device=dev)
        self.n_occupied = torch.full((1,), n, dtype=torch.int32, device=dev)

    @torch.no_grad()
    def update(self, density):
        """density (G,G,G) or (G^3,) fp32: ema = max(ema * decay, density) (the first update replaces +inf), bit = ema > thresh."""
        _lib.require_device(density)
        if density.dtype != torch.float32 or density.numel() != self.G ** 3 or tuple(density.shape) not in ((self.G,) * 3, (self.G ** 3,)):
            raise RuntimeError("lab4d_amd.occgrid.update needs a (G, G, G) or (G^3,) float32 density with G = %d, got %s %s"
                               % (self.G, density.dtype, tuple(density.shape)))
        _lib.call("occgrid_update", density, self.ema, self.bits, self.n_occupied, self.G, self.decay, self.thresh)
        return self

    @torch.no_grad()
    def mask(self, xyz):
        """xyz (S,3) world points -> uint8 (S,): 1 iff the point lies in the box and its cell's bit is set (what render_utils.compact takes)."""
        _f32("xyz", xyz, 3)
        xyz = xyz.detach()
        S = xyz.numel() // 3
        out = torch.empty(S, dtype=torch.uint8, device=xyz.device)
        _lib.call("occgrid_mask", xyz, self.aabb, self.bits, self.G, S, out)
        return out

    @torch.no_grad()
    def ray_span(self, origin, dir, t_range):
        """origin, dir (R,3), t_range (R,2) = [t0, t1] in the units of `dir` (depth, for sample_cam_rays-style rays) ->
        (t_span (R,2) = [t_first, t_last], hit (R,) bool).  Rays without an occupied cell: hit = False and both entries equal t0."""
        _f32("origin", origin, 3)
        _f32("dir", dir, 3)
        _f32("t_range", t_range, 2)
        R = origin.numel() // 3
        if dir.numel() != 3 * R or t_range.numel() != 2 * R:
            raise RuntimeError("lab4d_amd.occgrid.ray_span: origin %s, dir %s and t_range %s disagree on the number of rays"
                               % (tuple(origin.shape), tuple(dir.shape), tuple(t_range.shape)))
        t_span = torch.empty(R, 2, dtype=torch.float32, device=origin.device)
        hit = torch.empty(R, dtype=torch.uint8, device=origin.device)
        _lib.call("occgrid_ray_span", origin.detach(), dir.detach(), t_range.detach(), self.aabb, self.bits, self.G, R, t_span, hit)
        return t_span, hit.view(torch.bool)

    @torch.no_grad()
    def ray_depths(self, origin, dir, near_far, n_depth):
        """Depths for sample_cam_rays(depth=...): origin, dir (...,3) in the field's frame, near_far (...,2) or one pair per leading index
        ((M,2) for (M,N,3) rays) -> (depth (..., n_depth, 1), hit (...) bool).  A hit ray's depths are evenly spaced over its span, the first
        equal to t_first and the last to t_last; a ray without a hit keeps its original range (the caller masks it)."""
        _lib.require_device(origin, dir, near_far)
        origin = origin.contiguous()
        lead = origin.shape[:-1]
        nf = near_far
        while nf.ndim < origin.ndim:
            nf = nf.unsqueeze(-2)
        nf = nf.to(torch.float32).expand(*lead, 2).contiguous()
        span, hit = self.ray_span(origin.reshape(-1, 3), dir.expand_as(origin).contiguous().reshape(-1, 3), nf.reshape(-1, 2))
        rng = torch.where(hit[:, None], span, nf.reshape(-1, 2))
        z = torch.linspace(0, 1, int(n_depth), device=origin.device)[None]
        lo, hi = rng[:, 0:1], rng[:, 1:2]
        depth = torch.minimum(torch.maximum(lo * (1 - z) + hi * z, lo), hi)  # (the blend may round an ulp past an end)
        return depth.reshape(*lead, int(n_depth), 1).contiguous(), hit.reshape(lead)

    @torch.no_grad()
    def seed_from_mesh(self, verts, faces, band=0.0, grid=None):
        """Seed the grid from a mesh (verts (V,3) fp32, faces (F,3) int32 on the device) instead of waiting for the field's own density: the
        signed distance (lab4d_amd.meshsdf.signed_distance) at `cell_centers()` goes through `update()` as a density of 2 * thresh + 1
        where sdf <= band + half the cell diagonal, and 0 elsewhere.  The margin makes the seed conservative: the distance is 1-Lipschitz
        and no point of a cell is farther than half its diagonal from the centre, so every point of the box with sdf <= band lies in a
        cell whose bit is set.  The usual EMA carries on from there: later updates with the field's density decay the seed.
        grid: a lab4d_amd.meshray.MeshGrid of the mesh: the cell-centre query walks it (signed_distance(..., grid=grid)) instead of every
        face; default None: brute force, as before."""
        from . import meshsdf
        sdf = meshsdf.signed_distance(verts, faces, self.cell_centers(), grid=grid)
        half_diag = 0.5 * torch.linalg.vector_norm((self.aabb[1] - self.aabb[0]) / self.G)
        density = torch.where(sdf <= float(band) + half_diag, 2.0 * self.thresh + 1.0, 0.0).to(torch.float32)
        return self.update(density)

    def cell_centers(self):
        """(G^3, 3) world points, x slowest: lo + (i + 0.5) / G * (hi - lo)."""
        G = self.G
        ax = (torch.arange(G, device=self.aabb.device, dtype=torch.float32) + 0.5) / G
        lo, ext = self.aabb[0], self.aabb[1] - self.aabb[0]
        return (lo + torch.cartesian_prod(ax, ax, ax) * ext).contiguous()
