"""Signed distance from points to a triangle mesh on the device (include/lab4d_meshsdf.h, csrc/meshsdf.hip): the consumer of the meshes
of lab4d_amd/mesh.py and the device counterpart of the pysdf query behind NeRF.get_init_sdf_fn (nnutils/nerf.py:217-230).  Brute force,
every point against every face; the distance is the closest point by region classification, the sign the generalised winding number
(|w| > 0.5 is inside, whatever the orientation of the faces), negative inside.  The rules are written down in the header and in
csrc/meshsdf_math.hpp; parity with pysdf is unpinned.  Nothing here synchronises with the host."""
import torch

from . import _lib

WORK_WORDS = 6  # per (slice, point): d2, face, closest xyz, winding sum (include/lab4d_meshsdf.h, WORK)
_BLOCK = 256    # points per block = faces per tile
_FILL = 1024    # blocks that fill the chip: 256 compute units, 4 blocks of 4 waves each
_INDEX_LIMIT = 2 ** 31 - 1


def default_slices(n_pts, n_faces):
    """n_slices = max(1, min(ceil(F / 256), 1024 // ceil(N / 256))): enough slices that ceil(N / 256) * n_slices blocks reach 1024 (4 per
    compute unit), never a slice shorter than one 256-face tile.  256 points against 100k faces: 391 slices; 128^3 points: one."""
    pt_blocks = max(1, -(-int(n_pts) // _BLOCK))
    return max(1, min(-(-int(n_faces) // _BLOCK), _FILL // pt_blocks))


def work_words(n_pts, n_slices):
    """32-bit words of the work buffer: n_slices * n_pts * 6, none for one slice."""
    return 0 if n_slices == 1 else int(n_slices) * int(n_pts) * WORK_WORDS


def _check(verts, faces, pts):
    for name, t in (("verts", verts), ("faces", faces), ("pts", pts)):
        if not torch.is_tensor(t):
            raise RuntimeError("lab4d_amd.meshsdf: %s must be a device tensor, got %s" % (name, type(t).__name__))
    if verts.dtype != torch.float32 or verts.ndim != 2 or verts.shape[1] != 3:
        raise RuntimeError("lab4d_amd.meshsdf: verts must be float32 (V, 3), got %s %s" % (verts.dtype, tuple(verts.shape)))
    if faces.dtype != torch.int32 or faces.ndim != 2 or faces.shape[1] != 3:
        raise RuntimeError("lab4d_amd.meshsdf: faces must be int32 (F, 3), got %s %s%s"
                           % (faces.dtype, tuple(faces.shape), " (convert int64 faces with .to(torch.int32))" if faces.dtype == torch.int64 else ""))
    if pts.dtype != torch.float32 or pts.ndim < 1 or pts.shape[-1] != 3:
        raise RuntimeError("lab4d_amd.meshsdf: pts must be float32 (..., 3), got %s %s" % (pts.dtype, tuple(pts.shape)))
    _lib.require_device(verts, faces, pts)
    if faces.shape[0] > _INDEX_LIMIT // 3:
        raise RuntimeError("lab4d_amd.meshsdf: %d faces, must be below 2^31 / 3" % faces.shape[0])


@torch.no_grad()
def signed_distance(verts, faces, pts, n_slices=None, return_face=False, return_closest=False, work=None, grid=None):
    """verts (V,3) fp32, faces (F,3) int32, pts (...,3) fp32, all on the device -> sdf of shape pts.shape[:-1], negative inside; then, if
    asked for, face (the same shape, int32: the winning face, -1 without one) and closest (..., 3).  A non-finite point gives NaN, a mesh
    without a valid face +inf.
    n_slices: how many ways the faces are split across blocks; default `default_slices(N, F)` =
    max(1, min(ceil(F / 256), 1024 // ceil(N / 256))).  The distance, the face and the closest point do not depend on it.
    work: a preallocated float32 buffer of at least `work_words(N, n_slices)` elements (for graph capture: no allocation besides the
    outputs); default: allocated here.  Queries whose work buffer would pass 2^31 words run in chunks of points.
    grid: a lab4d_amd.meshray.MeshGrid built from these very `verts` and `faces` tensors (checked by storage and shape): the query goes
    through `grid.closest` (include/lab4d_meshnear.h) instead of every face -- the same distance, face and closest point word for word, the
    sign from the pseudonormal of the closest feature with the orientation taken from the mesh's signed volume (on a closed mesh the winding
    number's sign away from the surface; on an open one the side of the nearest feature).  n_slices and work are not used then.  Default
    None: brute force, as before."""
    _check(verts, faces, pts)
    if grid is not None:
        if not hasattr(grid, "closest") or (grid.verts.data_ptr(), grid.verts.shape, grid.faces.data_ptr(), grid.faces.shape) != (
                verts.data_ptr(), verts.shape, faces.data_ptr(), faces.shape):
            raise RuntimeError("lab4d_amd.meshsdf: grid must be a lab4d_amd.meshray.MeshGrid of this mesh, built from these verts and faces tensors "
                               "(%d vertices, %d faces): the same storage, not a copy" % (verts.shape[0], faces.shape[0]))
        near = grid.closest(pts.detach())
        out = (near.sdf,) + ((near.face,) if return_face else ()) + ((near.closest,) if return_closest else ())
        return out[0] if len(out) == 1 else out
    verts, faces, pts = verts.detach(), faces.detach(), pts.detach()
    lead = pts.shape[:-1]
    flat = pts.reshape(-1, 3)
    N, F = flat.shape[0], faces.shape[0]
    if n_slices is None:
        n_slices = default_slices(N, F)
    n_slices = int(n_slices)
    if not 1 <= n_slices <= 65535:
        raise RuntimeError("lab4d_amd.meshsdf: n_slices = %d outside [1, 65535]" % n_slices)
    chunk = _INDEX_LIMIT // (WORK_WORDS * n_slices)
    if work is not None:
        _lib.require_device(work)
        if work.dtype != torch.float32 or work.numel() < work_words(min(N, chunk), n_slices):
            raise RuntimeError("lab4d_amd.meshsdf: work must be float32 with at least n_slices * n_pts * 6 = %d elements, got %s %d"
                               % (work_words(min(N, chunk), n_slices), work.dtype, work.numel()))
    elif n_slices > 1 and N:
        work = torch.empty(work_words(min(N, chunk), n_slices), dtype=torch.float32, device=pts.device)
    sdf = torch.empty(N, dtype=torch.float32, device=pts.device)
    face = torch.empty(N, dtype=torch.int32, device=pts.device) if return_face else None
    closest = torch.empty(N, 3, dtype=torch.float32, device=pts.device) if return_closest else None
    for o in range(0, N, chunk):
        n = min(chunk, N - o)
        _lib.call("mesh_sdf", verts, faces, verts.shape[0], F, flat[o:o + n], n, n_slices, work if n_slices > 1 else None, sdf[o:o + n],
                  None if face is None else face[o:o + n], None if closest is None else closest[o:o + n])
    out = (sdf.reshape(lead),)
    if return_face:
        out += (face.reshape(lead),)
    if return_closest:
        out += (closest.reshape(*lead, 3),)
    return out[0] if len(out) == 1 else out
