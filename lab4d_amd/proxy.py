"""Proxy-geometry refresh on the device: the per-sample work of `NeRF.extract_canonical_mesh` -- the dense grid
query of the signed-distance field and the visibility field that feeds marching cubes (nnutils/nerf.py:303-343,
utils/geom_utils.py:392-476) -- and the bound updates that follow it, `NeRF.update_aabb` / `update_near_far`
(nerf.py:345-376, geom_utils.py:344-362).

The grid query is the chain kernels' inference mode (nothing stored, MFMA-bound): one "frame" of grid_size^3 samples under one
instance code, sdf head only (no density, no colour), then the visibility net.  Marching cubes is either the reference's CPU
`skimage.measure.marching_cubes` on the returned volume, or -- `extract_mesh` -- the device mesher of lab4d_amd/mesh.py on the volume
where it lies; the vertices / bounds of the new proxy mesh go into `update_aabb` / `update_near_far` here, which keep `aabb` and
`near_far` on the device."""
import torch

from . import deformable as DF
from . import mesh as _mesh
from . import meshsdf as _meshsdf
from . import mlp
from . import quat_utils as Q


def sample_grid(aabb, grid_size):
    """geom_utils.sample_grid (geom_utils.py:392-406): (grid_size^3, 3) points, x slowest (torch.cartesian_prod order)."""
    ax = [torch.linspace(float(aabb[0][i]), float(aabb[1][i]), grid_size, device=aabb.device) for i in range(3)]
    return torch.cartesian_prod(*ax)


@torch.no_grad()
def grid_query(P, aabb, grid_size=64, code_base=None, code_vis=None, prec=mlp.PREC_BF16, use_visibility=True, extend=0.5, chunk=1 << 22, alpha=None,
               kind="fg"):
    """The volume `marching_cubes` meshes (geom_utils.py:445-476): sdf (G,G,G) fp32 and visibility mask (G,G,G) bool over
    extend_aabb(aabb, extend) (extract_canonical_mesh's `use_extend_aabb`, nerf.py:333-336).  code_base / code_vis: (1,32) instance
    codes of the basefield / visibility CondMLPs -- `inst_embedding(inst_id)` or the mean embedding for inst_id=None
    (base.py:130-134); default: the mean of P's embedding tables.  alpha: the live annealing state `pos_embedding.alpha` of
    the field (embedding.py:112-125; MultiFields.set_alpha, multifields.py:108-116, ramps it over the first steps, and
    extract_canonical_mesh calls self.forward, which applies it; the visibility field's own embedding is never annealed); None = no window.
    kind: "fg" (NeRF W=256, D=8, 10 frequencies: LAB4D_NET_FG_BASE) or "bg" (multifields.py:86-93: W=128, D=5, 6 frequencies: LAB4D_NET_BG_BASE) --
    MultiFields.update_geometry_aux (trainer.py:247) and MultiFields.extract_canonical_meshes mesh EVERY field, the background included; both
    kinds carry the same VisField (95 -> 64 -> 64 -> 1).  Returns (sdf, vis, grid_aabb)."""
    net = {"fg": mlp.NET_FG_BASE, "bg": mlp.NET_BG_BASE}[kind]
    box = DF.extend_aabb(aabb, extend) if extend else aabb
    pts = sample_grid(box, grid_size)
    if code_base is None:
        code_base = P["basefield.inst_embedding.mapping.weight"].mean(0, keepdim=True)
    if code_vis is None:
        code_vis = P["vis_mlp.basefield.inst_embedding.mapping.weight"].mean(0, keepdim=True)
    sdf, vis = [], []
    fw = DF.posenc_window(alpha, mlp.describe(net).n_freq, pts.device)
    for i in range(0, pts.shape[0], chunk):  # eval_func_chunk (geom_utils.py:425-440); one chunk up to 128^3
        x = pts[i:i + chunk].contiguous()
        sdf.append(mlp.run_chain(net, prec, P, x, x.shape[0], conds={0: code_base, 4: code_base}, freq_w=fw))
        if use_visibility:
            vis.append(mlp.run_chain(mlp.NET_VIS, prec, P, x, x.shape[0], conds={0: code_vis}) > 0)
    G = grid_size
    sdf = torch.cat(sdf, 0).view(G, G, G)
    vis = torch.cat(vis, 0).view(G, G, G) if use_visibility else torch.ones(G, G, G, dtype=torch.bool, device=sdf.device)
    return sdf, vis, box


@torch.no_grad()
def extract_mesh(P, aabb, grid_size=64, level=0.0, code_base=None, code_vis=None, prec=mlp.PREC_BF16, use_visibility=True, extend=0.5, alpha=None,
                 kind="fg", largest_component=False, exact_spacing=False):
    """geom_utils.marching_cubes (geom_utils.py:442-503) without leaving the device: `grid_query` + lab4d_amd.mesh.marching_cubes on the two
    volumes (visibility as the mask: a cell is meshed iff all 8 of its corners are visible) + the bounds of the result.  Returns
    (verts (V, 3) float32, faces (F, 3) int32, bounds (2, 3) or None for an empty surface), all device tensors, so `update_aabb(aabb, bounds)`
    and `update_near_far(..., verts, ...)` can follow with no host copy of the mesh.  largest_component: the reference's
    apply_connected_component (fg fields, nerf.py:339-342).
    Spacing: the reference meshes with spacing = 1 / grid_size (geom_utils.py:486) and scales by the box (geom_utils.py:495), although
    sample_grid puts index grid_size - 1 on the far face of the box; its meshes are therefore shrunk by (G - 1) / G towards the low corner.
    exact_spacing=False (default) reproduces that: step = (hi - lo) / G; True puts the vertices where the samples were taken:
    step = (hi - lo) / (G - 1)."""
    sdf, vis, box = grid_query(P, aabb, grid_size, code_base=code_base, code_vis=code_vis, prec=prec, use_visibility=use_visibility, extend=extend,
                               alpha=alpha, kind=kind)
    step = (box[1] - box[0]) / float(grid_size - 1 if exact_spacing else grid_size)
    verts, faces = _mesh.marching_cubes(sdf.contiguous(), vis.contiguous() if use_visibility else None, level=level, origin=box[0], step=step,
                                        largest_component=largest_component)
    bounds = torch.stack([verts.min(0)[0], verts.max(0)[0]], 0) if verts.shape[0] else None
    return verts, faces, bounds


def init_sdf_fn(verts, faces, grid=False):
    """NeRF.get_init_sdf_fn (nerf.py:217-230) on the device: from a mesh (vertices (V,3), faces (F,3); tensors, or the numpy arrays of a
    trimesh.Trimesh / lab4d_amd.mesh.Mesh) the callable `pts (N,3) -> sdf (N,1)`, negative inside, that geometry_init fits the field to
    (nerf.py:251-295).  The reference builds a pysdf.SDF on the host and copies every batch of points there and back; here the mesh is
    moved to the points' device once and lab4d_amd.meshsdf.signed_distance answers in place.  grid=True: one lab4d_amd.meshray.MeshGrid per
    device is built next to the cached mesh and the query walks it (signed_distance(..., grid=...): the same distance, the sign from the
    pseudonormal of the closest feature); the default answers by brute force, as before."""
    cache, grids = {}, {}

    def mesh_on(device):
        if device not in cache:
            v = torch.as_tensor(verts).detach().to(device=device, dtype=torch.float32).reshape(-1, 3).contiguous()
            f = torch.as_tensor(faces).detach().to(device=device, dtype=torch.int32).reshape(-1, 3).contiguous()
            cache[device] = (v, f)
        return cache[device]

    def sdf_fn(pts):
        v, f = mesh_on(pts.device)
        if grid and pts.device not in grids:
            from . import meshray as _meshray
            grids[pts.device] = _meshray.MeshGrid(v, f)
        sdf = _meshsdf.signed_distance(v, f, pts.detach().to(torch.float32).contiguous(), grid=grids[pts.device] if grid else None)
        return sdf[..., None].to(pts.dtype)

    return sdf_fn


@torch.no_grad()
def ray_range(grid, origin, dir, t_range, band=0.0):
    """The per-ray sampling range the proxy mesh allows: `grid` is a lab4d_amd.meshray.MeshGrid of it, origin, dir (R, 3), t_range (R, 2) as
    for grid.cast.  Two casts: the first hit, and the last hit as the first hit of the reversed ray (o + t1 d, -d) over [0, t1 - t0], mapped back
    to t1 - t'.  Returns (t_range' (R, 2), hit (R,) bool): [t_first - band / |dir|, t_last + band / |dir|] cut to the given range (band: a
    metric length, e.g. one cell of the field, that covers the proxy's distance from the surface it stands for); a ray that misses the
    mesh gets the empty range of hashfield.trace_surface, [t0, -inf].  Feeds trace_surface, render_packed and sample_cam_rays(depth=...)."""
    first = grid.cast(origin, dir, t_range)
    t0, t1 = t_range[:, 0], t_range[:, 1]
    back = grid.cast((origin + t1[:, None] * dir).contiguous(), (-dir).contiguous(), torch.stack([torch.zeros_like(t0), t1 - t0], -1).contiguous())
    t_last = torch.where(back.hit, t1 - back.t, first.t)
    t_last = torch.maximum(t_last, first.t)  # (one surface seen from both ends may come back a rounding in front of itself)
    pad = float(band) / torch.linalg.vector_norm(dir, dim=-1)
    lo, hi = torch.maximum(t0, first.t - pad), torch.minimum(t1, t_last + pad)
    empty = torch.full_like(t1, -float("inf"))
    return torch.stack([torch.where(first.hit, lo, t0), torch.where(first.hit, hi, empty)], -1).contiguous(), first.hit


def grid_to_world(verts01, box):
    """marching_cubes' vertex transform from the unit cube to the box (geom_utils.py:492-493)."""
    return verts01 * (box[1:] - box[:1]) + box[:1]


@torch.no_grad()
def update_aabb(aabb, bounds, beta=0.9):
    """NeRF.update_aabb (nerf.py:345-356): EMA of the field's aabb towards the proxy mesh's bounds (2,3)."""
    return aabb * beta + bounds.to(aabb) * (1 - beta)


@torch.no_grad()
def get_near_far(pts, quat, trans, tol_fac=1.5):
    """geom_utils.get_near_far (geom_utils.py:344-362) with the object-to-camera transforms as (quat (M,4), trans (M,3)) -- the
    form CameraMLP.get_vals returns (the reference converts them to 4x4 matrices first, nerf.py:366-367): depth range of the proxy
    vertices in every camera, widened by (tol_fac - 1) of its extent, clamped at 1e-3."""
    z = DF.rigid_apply(quat, trans, pts[None].expand(quat.shape[0], -1, -1))[..., 2]
    pmax, pmin = z.max(-1)[0], z.min(-1)[0]
    delta = (pmax - pmin) * (tol_fac - 1)
    return torch.stack([pmin - delta, pmax + delta], -1).clamp(min=1e-3)


@torch.no_grad()
def update_near_far(near_far, frame_mapping, pts, quat, trans, beta=0.9):
    """NeRF.update_near_far (nerf.py:358-376): EMA of the per-frame near / far planes (rows `frame_mapping` of the (T_raw, 2) table)."""
    nf = get_near_far(pts, quat, trans)
    out = near_far.clone()
    out[frame_mapping] = near_far[frame_mapping] * beta + nf * (1 - beta)
    return out
