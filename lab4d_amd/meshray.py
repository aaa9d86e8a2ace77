"""Ray casting against a triangle mesh on the device (include/lab4d_meshray.h, csrc/meshray.hip): the first hit per ray of the meshes of
lab4d_amd/mesh.py, through a uniform face grid.  The watertight test of Woop, Benthin and Wald (2013); the smallest t wins, ties go to the
lowest face index, and the result does not depend on the grid.  The rules are written down in the header and in csrc/meshray_math.hpp; the
reference has no ray caster.  Building a grid reads one integer back from the device; casting synchronises with nothing and can be captured
in a hipGraph.  The same grid answers the closest point and the signed distance of query points (MeshGrid.closest: include/lab4d_meshnear.h,
csrc/meshnear.hip), word for word the distance of lab4d_amd.meshsdf at every G, with the sign from the pseudonormal of the closest feature."""
import collections
import math

import torch

from . import _lib

MAX_G = 128
PAD = 2.0 ** -10          # of a cell: the pad of a face's index box; of an extent: the margin of the default box
TRI_FLOATS = 12           # a packed face: {a xyz, valid}, {b xyz, 0}, {c xyz, 0}
_SCAN_BLOCK = 1024
_INDEX_LIMIT = 2 ** 31 - 1
FACES_PER_CELL_SQ = 13    # default_G: G = sqrt(F / 13), chosen from profiles/meshray.json


def default_G(n_faces):
    """G = clamp(round(sqrt(F / 13)), 1, 128): the faces of a surface spread over ~G^2 of the G^3 cells, so G grows with sqrt(F) to keep a
    cell's list at a few faces.  Chosen from the measurement of DESIGN.md section 7j (54,668 faces: G = 64 is the fastest of 16 / 32 / 64 /
    128); the result of a cast never depends on it."""
    return max(1, min(MAX_G, int(round(math.sqrt(max(int(n_faces), 0) / FACES_PER_CELL_SQ)))))


def work_ints(G):
    """32-bit words of the build's work buffer: G^3 + ceil(G^3 / 1024) (include/lab4d_meshray.h, Buffers)."""
    return G ** 3 + -(-G ** 3 // _SCAN_BLOCK)


def default_aabb(verts):
    """The vertices' bounds widened by 2^-10 of each extent, by 2^-10 of the largest extent on an axis with none (and by 2^-10 for a single
    point): (2, 3) float32 on the vertices' device.  Non-finite vertices are left out; no vertex: the unit box."""
    ok = torch.isfinite(verts).all(-1)
    if not bool(ok.any()):
        return torch.tensor([[0.0] * 3, [1.0] * 3], dtype=torch.float32, device=verts.device)
    v = verts[ok]
    lo, hi = v.min(0)[0], v.max(0)[0]
    ext = hi - lo
    big = ext.max()
    margin = torch.where(ext > 0, ext, big if float(big) > 0 else torch.ones_like(big)) * PAD
    return torch.stack([lo - margin, hi + margin], 0).contiguous()


def _check_mesh(verts, faces):
    for name, t in (("verts", verts), ("faces", faces)):
        if not torch.is_tensor(t):
            raise RuntimeError("lab4d_amd.meshray: %s must be a device tensor, got %s" % (name, type(t).__name__))
    if verts.dtype != torch.float32 or verts.ndim != 2 or verts.shape[1] != 3:
        raise RuntimeError("lab4d_amd.meshray: verts must be float32 (V, 3), got %s %s" % (verts.dtype, tuple(verts.shape)))
    if faces.dtype != torch.int32 or faces.ndim != 2 or faces.shape[1] != 3:
        raise RuntimeError("lab4d_amd.meshray: faces must be int32 (F, 3), got %s %s%s"
                           % (faces.dtype, tuple(faces.shape), " (convert int64 faces with .to(torch.int32))" if faces.dtype == torch.int64 else ""))
    if faces.shape[0] > _INDEX_LIMIT // TRI_FLOATS:
        raise RuntimeError("lab4d_amd.meshray: %d faces, must be at most 2^31 / 12" % faces.shape[0])


def _check_G(G):
    if not isinstance(G, int) or isinstance(G, bool) or not 1 <= G <= MAX_G:
        raise RuntimeError("lab4d_amd.meshray: G = %r outside [1, %d]" % (G, MAX_G))


def _check_rays(origin, dir, t_range):
    for name, t in (("origin", origin), ("dir", dir), ("t_range", t_range)):
        if not torch.is_tensor(t):
            raise RuntimeError("lab4d_amd.meshray: %s must be a device tensor, got %s" % (name, type(t).__name__))
    for name, t in (("origin", origin), ("dir", dir)):
        if t.dtype != torch.float32 or t.ndim != 2 or t.shape[1] != 3:
            raise RuntimeError("lab4d_amd.meshray: %s must be float32 (R, 3), got %s %s" % (name, t.dtype, tuple(t.shape)))
    R = origin.shape[0]
    if R >= 1 << 31:
        raise RuntimeError("lab4d_amd.meshray: %d rays, must be below 2^31" % R)
    if dir.shape[0] != R or t_range.dtype != torch.float32 or tuple(t_range.shape) != (R, 2):
        raise RuntimeError("lab4d_amd.meshray: origin %s, dir %s and t_range %s %s disagree: R rays need float32 (R, 3), (R, 3) and (R, 2)"
                           % (tuple(origin.shape), tuple(dir.shape), t_range.dtype, tuple(t_range.shape)))
    _lib.require_device(origin, dir, t_range)


class Hits(collections.namedtuple("Hits", "t face u v front n_tests hit")):
    """The first hit of every ray: t (R,) float32 (t0 where there is none), face (R,) int32 (-1 without a hit), u, v (R,) the barycentric weights
    of the face's second and third vertex, front (R,) int32 = 1 where the ray meets the side (b - a) x (c - a) points to, n_tests (R,) int32
    the face tests the ray made, hit (R,) bool = face >= 0."""
    __slots__ = ()

    def _corners(self, verts, faces):
        tri = verts[faces.long()[self.face.clamp(min=0).long()]]  # (R, 3, 3): a plain gather, differentiable in verts
        return tri[:, 0], tri[:, 1], tri[:, 2]

    def xyz(self, verts, faces):
        """(R, 3): the hit point a + u (b - a) + v (c - a) on the hit face, differentiable in verts; exact zeros for missed rays."""
        a, b, c = self._corners(verts, faces)
        p = a + self.u[:, None] * (b - a) + self.v[:, None] * (c - a)
        return torch.where(self.hit[:, None], p, torch.zeros_like(p))

    def normal(self, verts, faces):
        """(R, 3): the unit normal (b - a) x (c - a) of the hit face as the mesh orients it (not flipped towards the ray: see `front`),
        differentiable in verts; exact zeros for missed rays."""
        a, b, c = self._corners(verts, faces)
        n = torch.cross(b - a, c - a, dim=-1)
        n = n / torch.where(self.hit, torch.linalg.vector_norm(n, dim=-1), torch.ones_like(self.t))[:, None]
        return torch.where(self.hit[:, None], n, torch.zeros_like(n))


class Nearest(collections.namedtuple("Nearest", "sdf d2 face closest region n_tests")):
    """The closest point of the mesh to every query point, shaped like pts.shape[:-1]: sdf float32 (negative inside with a sign, the plain
    distance without; NaN for a non-finite point, +inf without a valid face), d2 float32 its square as the walk compared it, face int32 (-1
    without one), closest (..., 3) float32 (the point itself without a face), region int32 (0 the face, 1 / 2 / 3 the edge ab / ac / bc,
    4 / 5 / 6 the vertex a / b / c of `face`; -1 without one), n_tests int32 the face tests the point made."""
    __slots__ = ()

    def xyz(self, verts, faces):
        """(..., 3): the closest point rebuilt as a + v (b - a) + w (c - a) on the winning face, differentiable in verts.  The weights are
        recovered from `closest` with torch ops (the least-squares weights of closest - a in the face's two edges, held constant); exact
        zeros where face < 0."""
        ok = self.face >= 0
        tri = verts[faces.long()[self.face.clamp(min=0).long()]]  # (..., 3, 3): a plain gather, differentiable in verts
        a, b, c = tri[..., 0, :], tri[..., 1, :], tri[..., 2, :]
        with torch.no_grad():
            e1, e2, d = (b - a).double(), (c - a).double(), (self.closest - a).double()
            g11, g12, g22 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
            r1, r2 = (e1 * d).sum(-1), (e2 * d).sum(-1)
            det = g11 * g22 - g12 * g12
            det = torch.where(ok & (det > 0), det, torch.ones_like(det))
            v = torch.where(ok, (g22 * r1 - g12 * r2) / det, torch.zeros_like(det)).float()  # (a point without a face: no NaN reaches the graph)
            w = torch.where(ok, (g11 * r2 - g12 * r1) / det, torch.zeros_like(det)).float()
        p = a + v[..., None] * (b - a) + w[..., None] * (c - a)
        return torch.where(ok[..., None], p, torch.zeros_like(p))


class MeshGrid:
    """The face grid of a mesh: verts (V, 3) float32, faces (F, 3) int32 on the device; G^3 cells over aabb (2, 3) (default: `default_aabb`,
    the vertices' bounds with a margin; default G: `default_G(F)`).  Keeps the packed faces and the cells' lists; `rebuild()` after the
    vertices moved (a cast against stale lists may miss faces that left their cells).  The constructor reads the list's length back from the
    device (once) and cannot run under stream capture."""

    def __init__(self, verts, faces, G=None, aabb=None):
        _check_mesh(verts, faces)
        _lib.require_device(verts, faces)
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("lab4d_amd.meshray: the length of the cell lists depends on the data (a host read-back); a MeshGrid cannot be built under "
                               "stream capture")
        self.verts, self.faces = verts.detach(), faces.detach()
        self.n_faces = int(faces.shape[0])
        self.G = default_G(self.n_faces) if G is None else G
        _check_G(self.G)
        if aabb is None:
            aabb = default_aabb(self.verts)
        if not torch.is_tensor(aabb) or aabb.dtype != torch.float32 or tuple(aabb.shape) != (2, 3):
            raise RuntimeError("lab4d_amd.meshray: aabb must be float32 (2, 3), got %s"
                               % ("%s %s" % (aabb.dtype, tuple(aabb.shape)) if torch.is_tensor(aabb) else type(aabb).__name__))
        _lib.require_device(aabb)
        lo, hi = aabb.tolist()
        if not all(math.isfinite(a) and math.isfinite(b) and b > a for a, b in zip(lo, hi)):
            raise RuntimeError("lab4d_amd.meshray: aabb %s must be finite with hi > lo on every axis" % (aabb.tolist(),))
        self.aabb = aabb.detach().clone()
        dev = verts.device
        n_cells = self.G ** 3
        self.tris = torch.empty(self.n_faces * TRI_FLOATS, dtype=torch.float32, device=dev)
        self.cell_start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
        self._work = torch.empty(work_ints(self.G), dtype=torch.int32, device=dev)
        self._total = torch.zeros(1, dtype=torch.int32, device=dev)
        self.cell_list = torch.empty(0, dtype=torch.int32, device=dev)
        self._facts = None  # (orient, covered) of `closest`: computed on its first call, dropped by rebuild()
        self.rebuild()

    @torch.no_grad()
    def rebuild(self):
        """Packs the faces and bins them again from the vertices as they are now.  One read-back; not under stream capture."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("lab4d_amd.meshray: the length of the cell lists depends on the data (a host read-back); a MeshGrid cannot be built under "
                               "stream capture")
        self._facts = None
        if self.n_faces == 0:
            return self
        _lib.call("meshgrid_count", self.verts, self.faces, self.verts.shape[0], self.n_faces, self.aabb, self.G, self.tris, self.cell_start, self._work,
                  self._total)
        total = int(self._total.item())
        if total < 0:
            raise RuntimeError("lab4d_amd.meshray: the cell lists of %d faces at G = %d pass 2^31 entries; lower G" % (self.n_faces, self.G))
        if self.cell_list.numel() != total:
            self.cell_list = torch.empty(total, dtype=torch.int32, device=self.verts.device)
        _lib.call("meshgrid_fill", self.tris, self.n_faces, self.aabb, self.G, self.cell_start, self._work, total, self.cell_list)
        return self

    @torch.no_grad()
    def repack(self):
        """Packs the faces again from the vertices as they are now and leaves the lists alone: right as long as every face still touches the
        cells that list it (always at G = 1 while the faces stay inside aabb).  No read-back, no allocation: capturable, unlike rebuild()."""
        _lib.call("meshgrid_pack", self.verts, self.faces, self.verts.shape[0], self.n_faces, self.tris)
        return self

    @torch.no_grad()
    def cast(self, origin, dir, t_range):
        """origin, dir (R, 3), t_range (R, 2) = [t0, t1] in the units of `dir` (of any length), float32 on the device -> Hits.  A ray with a
        non-finite value, t0 > t1 or |dir| == 0 is rejected: face -1, t = t0, n_tests 0.  No gradients (Hits.xyz / Hits.normal carry the
        gradient in the vertices); no allocation besides the outputs."""
        _check_rays(origin, dir, t_range)
        R, dev = origin.shape[0], origin.device
        t, u, v = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(3))
        face, front, n_tests = (torch.empty(R, dtype=torch.int32, device=dev) for _ in range(3))
        with _lib.timed("k_mesh_raycast"):
            _lib.call("mesh_raycast", origin.detach(), dir.detach(), t_range.detach(), R, self.tris, self.n_faces, self.aabb, self.G, self.cell_start,
                      self.cell_list, t, face, u, v, front, n_tests)
        return Hits(t, face, u, v, front, n_tests, face >= 0)

    def _mesh_facts(self):
        """(orient, covered), once per build and with one read-back.  orient: the sign of the float64 signed volume sum det[a - m, b - m, c - m]
        over the valid faces, m the mean of their vertices (+1 for zero): +1 when (b - a) x (c - a) points outward.  covered: aabb contains
        the bounds of the finite vertices (a face outside the box is listed nowhere, and `closest` would silently ignore it)."""
        if self._facts is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("lab4d_amd.meshray: the orientation and the coverage of the mesh are read back from the device on the first call of "
                                   "closest(); call it once (or grid.orientation()) before the stream capture")
            with torch.no_grad():
                orient, covered = 1.0, 1.0
                if self.n_faces:
                    valid = self.tris.view(-1, 12)[:, 3] != 0
                    tri = self.tris.view(-1, 3, 4)[valid][:, :, :3].double()
                    if tri.shape[0]:
                        t = tri - tri.reshape(-1, 3).mean(0)
                        vol = (t[:, 0] * torch.linalg.cross(t[:, 1], t[:, 2])).sum()
                        orient = torch.where(vol < 0, -1.0, 1.0)
                ok = torch.isfinite(self.verts).all(-1)
                if self.verts.shape[0]:
                    big = torch.full((3,), float("inf"), device=self.verts.device)
                    lo = torch.where(ok[:, None], self.verts, big).min(0)[0]
                    hi = torch.where(ok[:, None], self.verts, -big).max(0)[0]
                    covered = ((lo >= self.aabb[0]) & (hi <= self.aabb[1])).all()  # (no finite vertex: inf >= lo and -inf <= hi hold)
                both = torch.stack([torch.as_tensor(orient, dtype=torch.float64, device=self.verts.device),
                                    torch.as_tensor(covered, dtype=torch.float64, device=self.verts.device)]).tolist()
            self._facts = (1 if both[0] >= 0 else -1, bool(both[1]))
        return self._facts

    def orientation(self):
        """+1 when the faces' normals (b - a) x (c - a) point outward, -1 inward: `closest`'s orient="auto".  Cached until rebuild()."""
        return self._mesh_facts()[0]

    @torch.no_grad()
    def closest(self, pts, sign="pseudonormal", orient="auto"):
        """pts (..., 3) float32 on the device -> Nearest(sdf, d2, face, closest, region, n_tests), each shaped like pts.shape[:-1].  d2, face
        and closest are word for word those of lab4d_amd.meshsdf.signed_distance, whatever G.  sign="pseudonormal": sdf < 0 inside, from the
        pseudonormal of the closest face, edge or vertex (on an open mesh: the side of the nearest feature, not meshsdf's winding number);
        sign=None: the plain distance.  orient: +1 / -1 when (b - a) x (c - a) points outward / inward, "auto": the sign of the mesh's signed
        volume (one read-back on the first call, cached until rebuild(); refused under stream capture unless cached).  A grid whose aabb
        does not hold the finite vertices is refused.  No gradients (Nearest.xyz carries the gradient in the vertices); no allocation
        besides the outputs.  Measured (profiles/meshnear.json: 54,668 faces, 128^3 points in the box): the fastest G for
        distance queries is the coarsest tried, 16 (227 ms; 1,227 ms at 64; brute force 569 ms), not `default_G` (65 there), which suits rays; for a
        few hundred points, or points outside the box, brute-force meshsdf.signed_distance is faster."""
        if not torch.is_tensor(pts):
            raise RuntimeError("lab4d_amd.meshray: pts must be a device tensor, got %s" % type(pts).__name__)
        if pts.dtype != torch.float32 or pts.ndim < 1 or pts.shape[-1] != 3:
            raise RuntimeError("lab4d_amd.meshray: pts must be float32 (..., 3), got %s %s" % (pts.dtype, tuple(pts.shape)))
        if sign not in ("pseudonormal", None):
            raise RuntimeError("lab4d_amd.meshray: sign = %r is neither 'pseudonormal' nor None" % (sign,))
        if not (orient == "auto" or (isinstance(orient, int) and not isinstance(orient, bool) and orient in (1, -1))):
            raise RuntimeError("lab4d_amd.meshray: orient = %r is not 'auto', +1 or -1" % (orient,))
        _lib.require_device(pts)
        lead = pts.shape[:-1]
        N = pts.numel() // 3
        if N >= 1 << 31:
            raise RuntimeError("lab4d_amd.meshray: %d points, must be below 2^31" % N)
        auto, covered = self._mesh_facts()
        if not covered:
            raise RuntimeError("lab4d_amd.meshray: aabb %s does not contain the mesh's vertices; a face outside the box is listed in no cell and "
                               "closest() would ignore it: build the grid over a box that holds the mesh (the default does)" % (self.aabb.tolist(),))
        dev = pts.device
        sdf, d2 = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2))
        face, region, n_tests = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
        closest = torch.empty(N, 3, dtype=torch.float32, device=dev)
        with _lib.timed("k_mesh_closest"):
            _lib.call("mesh_closest", pts.detach().reshape(-1, 3), N, self.tris, self.n_faces, self.aabb, self.G, self.cell_start, self.cell_list,
                      0 if sign is None else 1, auto if orient == "auto" else orient, sdf, d2, face, closest, region, n_tests)
        return Nearest(sdf.reshape(lead), d2.reshape(lead), face.reshape(lead), closest.reshape(*lead, 3), region.reshape(lead), n_tests.reshape(lead))
