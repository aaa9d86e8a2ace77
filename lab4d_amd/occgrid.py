"""Occupancy bit grid of the hash field (include/lab4d_occgrid.h, csrc/occgrid.hip): a bit per cell of a G^3 grid over the field's box,
refreshed from the field's own density (hashfield.update_occupancy), consulted per sample (`mask`: the compaction mask of
hashfield.forward_compacted) and per ray (`ray_span` / `ray_depths`: march only between the first and the last occupied cell).  The
reference has no counterpart (nnutils/nerf.py:98 is a TODO); the rules are written down in the header and in csrc/occgrid_math.hpp.
OccupancyCascade is K such grids around one centre, each twice the extent of the one before, for a scene box many times as wide as the
object (include/lab4d_conemarch.h, csrc/conemarch.hip): what packed.march_cone marches through.  Nothing here synchronises with the host: every call can be captured in a hipGraph."""
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


class OccupancyCascade:
    """A cascade of K occupancy grids around one centre (include/lab4d_conemarch.h, csrc/conemarch.hip): level c covers centre +- half extent *
    2^c of the base box `aabb` (2, 3) -- computed in float64, rounded once to fp32 -- with the same G cells per axis, so the cells double with
    every level.  aabbs (K, 6) = {lo xyz, hi xyz} per level, bits (K, ceil(G^3 / 32)) int32 words in OccupancyGrid's layout, ema (K, G^3),
    n_occupied (K,) int32.  A new cascade knows nothing: every bit is set and ema = +inf.  1 <= K <= 8; G must be even when K > 1.
    `packed.march_cone` marches through it; `level_grid(c)` is level c as a plain OccupancyGrid on the same storage."""

    def __init__(self, aabb, K=4, G=128, decay=0.95, thresh=0.01):
        K, G = int(K), int(G)
        if not 1 <= K <= 8:
            raise RuntimeError("lab4d_amd.occgrid: K = %d outside [1, 8]" % K)
        if not 2 <= G <= 256:
            raise RuntimeError("lab4d_amd.occgrid: G = %d outside [2, 256]" % G)
        if K > 1 and G % 2:
            raise RuntimeError("lab4d_amd.occgrid: G = %d must be even with K = %d > 1 levels" % (G, K))
        if not torch.is_tensor(aabb):
            raise RuntimeError("lab4d_amd.occgrid: aabb must be a (2, 3) device tensor")
        _lib.require_device(aabb)
        if tuple(aabb.shape) != (2, 3):
            raise RuntimeError("lab4d_amd.occgrid: aabb must be (2, 3), got %s" % (tuple(aabb.shape),))
        self.K, self.G, self.decay, self.thresh = K, G, float(decay), float(thresh)
        box = aabb.detach().to(torch.float64)  # (a device tensor stays on the device: no host copy of the box)
        dev = box.device
        mid, half = (box[0] + box[1]) / 2, (box[1] - box[0]) / 2
        scale = torch.tensor([float(1 << c) for c in range(K)], dtype=torch.float64, device=dev)[:, None]
        self.aabbs = torch.cat([mid - half * scale, mid + half * scale], 1).to(torch.float32).contiguous()
        n = G ** 3
        self.bits = torch.full((K, (n + 31) // 32), -1, dtype=torch.int32, device=dev)
        if n % 32:
            self.bits[:, -1] = (1 << (n % 32)) - 1  # the unused bits of the last word are zero
        self.ema = torch.full((K, n), float("inf"), dtype=torch.float32, device=dev)
        self.n_occupied = torch.full((K,), n, dtype=torch.int32, device=dev)

    def level_grid(self, c):
        """Level c as an OccupancyGrid that SHARES the cascade's storage (aabb, bits, ema, n_occupied are views): whatever takes a grid --
        update, mask, ray_span, seed_from_mesh, packed.march -- works on the level, and what it writes is the cascade's."""
        c = int(c)
        if not 0 <= c < self.K:
            raise RuntimeError("lab4d_amd.occgrid: level %d outside [0, %d)" % (c, self.K))
        grid = OccupancyGrid.__new__(OccupancyGrid)
        grid.G, grid.decay, grid.thresh = self.G, self.decay, self.thresh
        grid.aabb, grid.bits, grid.ema, grid.n_occupied = self.aabbs[c].view(2, 3), self.bits[c], self.ema[c], self.n_occupied[c:c + 1]
        return grid

    def cell_centers(self):
        """(K, G^3, 3) world points, x slowest within a level"""
        return torch.stack([self.level_grid(c).cell_centers() for c in range(self.K)])

    @torch.no_grad()
    def propagate(self, density):
        """The propagation rule of `update` alone: density (K, G^3) fp32 -> (K, G^3) with NaN and negative values as 0 and, for c >= 1, the
        block of level c that level c - 1 covers raised to the 2 x 2 x 2 max-pool of level c - 1's (already propagated) density.  With G a
        multiple of 4 that block is the central (G/2)^3 one; otherwise the child cells straddle the parents' faces by one cell, and level
        c - 1 is padded by one empty cell on every side before the pool.  A density of +inf counts as the largest finite value: an ema of
        +inf means "nothing known yet" to the update, which would drop the cell's history at the next update on one level and not on the
        other.  Torch ops on the device; nothing is read back."""
        K, G = self.K, self.G
        d = torch.where(density > 0, density.clamp(max=torch.finfo(torch.float32).max), torch.zeros_like(density)).reshape(K, G, G, G).clone()
        pad = 1 if G % 4 else 0
        Gp = G + 2 * pad
        o, n = (G - 2 * pad) // 4, Gp // 2
        for c in range(1, K):
            child = torch.nn.functional.pad(d[c - 1], (pad,) * 6) if pad else d[c - 1]
            pooled = child.reshape(n, 2, n, 2, n, 2).amax((1, 3, 5))
            block = d[c, o:o + n, o:o + n, o:o + n]
            block.copy_(torch.maximum(block, pooled))
        return d.reshape(K, G ** 3)

    @torch.no_grad()
    def update(self, density):
        """density (K, G^3) or (K, G, G, G) fp32, level c at cell_centers()[c]: `propagate`, then OccupancyGrid.update per level (one
        lab4d_occgrid_update call each: ema = max(ema * decay, density), bit = ema > thresh).  With the same decay on every level ema_c stays
        >= the pool of ema_{c-1}: a coarse bit is set wherever one of its eight children is."""
        _lib.require_device(density)
        if density.dtype != torch.float32 or density.shape[0] != self.K or density.numel() != self.K * self.G ** 3:
            raise RuntimeError("lab4d_amd.occgrid.OccupancyCascade.update needs a (K, G^3) float32 density with K = %d, G = %d, got %s %s"
                               % (self.K, self.G, density.dtype, tuple(density.shape)))
        d = self.propagate(density.reshape(self.K, -1))
        for c in range(self.K):
            self.level_grid(c).update(d[c])
        return self

    @torch.no_grad()
    def mask(self, xyz, delta=None):
        """xyz (S,3) world points, delta (S,) the world length of each point's step (None: 0) -> (mask (S,) uint8, level (S,) int32): the
        LEVEL rule of include/lab4d_conemarch.h per point; level = -1 where the point has no cell in any box."""
        _f32("xyz", xyz, 3)
        xyz = xyz.detach()
        S = xyz.numel() // 3
        if delta is not None:
            _lib.require_device(delta)
            if delta.dtype != torch.float32 or delta.numel() != S:
                raise RuntimeError("lab4d_amd.occgrid.OccupancyCascade.mask: delta must be float32 (%d,), got %s %s" % (S, delta.dtype, tuple(delta.shape)))
            delta = delta.detach()
        out = torch.empty(S, dtype=torch.uint8, device=xyz.device)
        level = torch.empty(S, dtype=torch.int32, device=xyz.device)
        _lib.call("occgrid_cascade_mask", xyz, delta, self.aabbs, self.bits, self.K, self.G, S, out, level)
        return out, level
