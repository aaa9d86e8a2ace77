"""Occupancy bit grid of the hash field (include/lab4d_occgrid.h, csrc/occgrid.hip): a bit per cell of a G^3 grid over the field's box,
refreshed from the field's own density (hashfield.update_occupancy), consulted per sample (`mask`: the compaction mask of
hashfield.forward_compacted) and per ray (`ray_span` / `ray_depths`: march only between the first and the last occupied cell).  The
reference has no counterpart (nnutils/nerf.py:98 is a TODO); the rules are written down in the header and in csrc/occgrid_math.hpp.
OccupancyCascade is K such grids around one centre, each twice the extent of the one before, for a scene box many times as wide as the
object (include/lab4d_conemarch.h, csrc/conemarch.hip): what packed.march_cone marches through.  `camera_planes` and `cull_invisible` clear the cells that no training camera sees
(include/lab4d_occvis.h, csrc/occvis.hip), for good: a later update applies the cull again.  Nothing here synchronises with the host: every
call can be captured in a hipGraph."""
import torch

from . import _lib


def _f32(name, t, *shape_tail):
    _lib.require_device(t)
    if t.dtype != torch.float32 or t.ndim < 1 or tuple(t.shape[-len(shape_tail):]) != shape_tail:
        raise RuntimeError("lab4d_amd.occgrid: %s must be float32 (..., %s), got %s %s" % (name, ", ".join(map(str, shape_tail)), t.dtype, tuple(t.shape)))


def camera_planes(Kmat, field2cam, wh, near, far=None, pad=0.0):
    """The six half-spaces of M camera frusta in the field's frame (VIEWS and CAMERA of include/lab4d_occvis.h): Kmat (M, 4) = {fx, fy, cx, cy},
    field2cam (M, 4, 4) or (M, 3, 4) = [R | t] with x_cam = R x_field + t, wh = (W, H) pixels, near and far depths (far None: no far plane,
    encoded as (0, 0, 0, 1)), pad in pixels widens the image on every side.  -> planes (M, 6, 4) fp32 = {nx, ny, nz, d}, unit normals, a point
    is inside iff n.x + d >= 0; order left, right, top, bottom, near, far.  Torch ops in float64 on the inputs' device (no kernel: a host tensor
    gives host planes), rounded to fp32 once."""
    M = Kmat.shape[0]
    if Kmat.ndim != 2 or Kmat.shape[1] != 4 or field2cam.ndim != 3 or field2cam.shape[0] != M or tuple(field2cam.shape[1:]) not in ((4, 4), (3, 4)):
        raise RuntimeError("lab4d_amd.occgrid.camera_planes: Kmat must be (M, 4) and field2cam (M, 4, 4) or (M, 3, 4), got %s and %s"
                           % (tuple(Kmat.shape), tuple(field2cam.shape)))
    W, H = float(wh[0]), float(wh[1])
    near, pad = float(near), float(pad)
    Kd, E = Kmat.detach().to(torch.float64), field2cam.detach().to(torch.float64)
    fx, fy, cx, cy = Kd.unbind(1)
    zero, one = torch.zeros_like(fx), torch.ones_like(fx)
    rows = [(fx, zero, cx + pad, zero), (-fx, zero, W + pad - cx, zero), (zero, fy, cy + pad, zero), (zero, -fy, H + pad - cy, zero),
            (zero, zero, one, zero - near)]
    if far is not None:
        rows.append((zero, zero, -one, zero + float(far)))
    cam = torch.stack([torch.stack(r, -1) for r in rows], 1)  # (M, 5 | 6, 4) in the camera frame
    x, y, z = cam[..., 0], cam[..., 1], cam[..., 2]
    cam = cam / torch.sqrt(x * x + y * y + z * z)[..., None]
    x, y, z, d_c = cam.unbind(-1)
    R, t = E[:, :3, :3], E[:, :3, 3]
    # n_w = R^T n_c, d_w = n_c . t + d_c, every sum from left to right (the float64 statement of the tests adds in the same order)
    n_w = [R[:, None, 0, i] * x + R[:, None, 1, i] * y + R[:, None, 2, i] * z for i in range(3)]
    d_w = x * t[:, None, 0] + y * t[:, None, 1] + z * t[:, None, 2] + d_c
    planes = torch.stack(n_w + [d_w], -1)
    if far is None:
        open_far = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=planes.device).expand(M, 1, 4)
        planes = torch.cat([planes, open_far], 1)
    return planes.to(torch.float32).contiguous()


def _mark_visible(planes, aabbs, K, G, min_views):
    """lab4d_occvis_mark on K boxes: (vis_bits (K, words) int32, n_visible (K,) int32)"""
    _lib.require_device(planes)
    if planes.dtype != torch.float32 or planes.ndim != 3 or tuple(planes.shape[1:]) != (6, 4) or planes.shape[0] < 1:
        raise RuntimeError("lab4d_amd.occgrid.cull_invisible: planes must be float32 (M >= 1, 6, 4), got %s %s" % (planes.dtype, tuple(planes.shape)))
    M, min_views = planes.shape[0], int(min_views)
    if not 1 <= min_views <= M:
        raise RuntimeError("lab4d_amd.occgrid.cull_invisible: min_views = %d outside [1, M = %d]" % (min_views, M))
    vis = torch.empty(K, (G ** 3 + 31) // 32, dtype=torch.int32, device=planes.device)
    n_vis = torch.empty(K, dtype=torch.int32, device=planes.device)
    _lib.call("occvis_mark", planes.detach(), M, aabbs, K, G, min_views, vis, n_vis)
    return vis, n_vis


def unpack_bits(words, G):
    """(..., ceil(G^3 / 32)) int32 words in the GRID layout -> (..., G^3) bool.  Torch ops on the device."""
    shifts = torch.arange(32, device=words.device, dtype=torch.int32)
    return ((words[..., None] >> shifts) & 1).bool().reshape(*words.shape[:-1], -1)[..., :G ** 3]


def pack_bits(flags):
    """(..., n) bool -> (..., ceil(n / 32)) int32 words in the GRID layout (the padding bits zero).  Torch ops on the device."""
    n = flags.shape[-1]
    f = torch.nn.functional.pad(flags.to(torch.int64), (0, -n % 32)).reshape(*flags.shape[:-1], -1, 32)
    w = (f << torch.arange(32, device=flags.device, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


class OccupancyGrid:
    """bits (ceil(G^3/32),) int32 words (bit idx & 31 of word idx >> 5, idx = (i*G + j)*G + k, x slowest), ema (G^3,) fp32, n_occupied (1,)
    device int32.  A new grid knows nothing: every bit is set, ema = +inf, and its mask is the box test alone.  visible (words,) int32 and
    n_visible (1,) int32 are None until `cull_invisible` sets them."""
    visible = None
    n_visible = None

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
        if self.visible is not None:  # a culled cell stays culled: no refresh revives it
            _lib.call("occvis_apply", self.visible, self.ema, self.bits, self.n_occupied, 1, self.G)
        return self

    @torch.no_grad()
    def cull_invisible(self, planes, min_views=1):
        """Clears the cells that fewer than `min_views` of the views `planes` (M, 6, 4) (camera_planes) see -- the rule of
        include/lab4d_occvis.h: a cell is kept unless its box lies wholly outside one of a view's six half-spaces, so every point a view
        sees lies in a kept cell.  Stores the mark as `visible` (words, the layout of `bits`) and `n_visible` (1,), then bits &= visible,
        ema = 0 on the invisible cells ("known empty") and n_occupied is recounted.  `update` applies the mark again from then on."""
        vis, n_vis = _mark_visible(planes, self.aabb.reshape(1, 6), 1, self.G, min_views)
        self.visible, self.n_visible = vis[0], n_vis
        _lib.call("occvis_apply", self.visible, self.ema, self.bits, self.n_occupied, 1, self.G)
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
    `packed.march_cone` marches through it; `level_grid(c)` is level c as a plain OccupancyGrid on the same storage.  visible (K, words) int32
    and n_visible (K,) int32 are None until `cull_invisible` sets them."""
    visible = None
    n_visible = None

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
        if self.visible is not None:
            grid.visible, grid.n_visible = self.visible[c], self.n_visible[c:c + 1]
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
            _lib.call("occgrid_update", d[c], self.ema[c], self.bits[c], self.n_occupied[c:c + 1], self.G, self.decay, self.thresh)
        if self.visible is not None:  # a culled cell stays culled: one apply for all K levels behind the update kernels
            _lib.call("occvis_apply", self.visible, self.ema, self.bits, self.n_occupied, self.K, self.G)
        return self

    @torch.no_grad()
    def cull_invisible(self, planes, min_views=1):
        """OccupancyGrid.cull_invisible on every level (one lab4d_occvis_mark launch for all K boxes, one lab4d_occvis_apply).  Between
        the two the visible set of level c is raised to contain the 2 x 2 x 2 pool of level c - 1's (`propagate` on the unpacked marks),
        so that the parent property `update` documents survives the cull: a coarse bit is set wherever one of its eight children is, also
        where G is no multiple of 4.  (The box test alone nearly gives that -- a parent's box contains its children's -- but not to the
        last rounding.)  `visible` (K, words) and `n_visible` (K,) hold the raised marks; level_grid(c) shares them."""
        vis, n_vis = _mark_visible(planes, self.aabbs, self.K, self.G, min_views)
        if self.K > 1:
            flags = self.propagate(unpack_bits(vis, self.G).to(torch.float32)) > 0
            vis, n_vis = pack_bits(flags).contiguous(), flags.sum(1).to(torch.int32)
        self.visible, self.n_visible = vis, n_vis
        _lib.call("occvis_apply", self.visible, self.ema, self.bits, self.n_occupied, self.K, self.G)
        return self

    @torch.no_grad()
    def refresh_set(self):
        """(K, G^3) bool: the cells whose density can reach the ema of a visible cell through `propagate` -- the visible cells and every
        cell below a visible cell of a coarser level (the propagation runs from fine to coarse, so an invisible child raises a visible
        parent).  What hashfield.update_occupancy_cascade(visible_only=True) evaluates; None visible: every cell."""
        K, G = self.K, self.G
        if self.visible is None:
            return torch.ones(K, G ** 3, dtype=torch.bool, device=self.bits.device)
        need = unpack_bits(self.visible, G).reshape(K, G, G, G).clone()
        pad = 1 if G % 4 else 0
        o, n = (G - 2 * pad) // 4, (G + 2 * pad) // 2
        for c in range(K - 2, -1, -1):  # the block of level c + 1 that covers level c, each cell over its 2 x 2 x 2 children (see propagate)
            block = need[c + 1, o:o + n, o:o + n, o:o + n]
            below = block.repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2)
            need[c] |= below[pad:pad + G, pad:pad + G, pad:pad + G]
        return need.reshape(K, G ** 3)

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
