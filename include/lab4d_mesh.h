/*
 * lab4d_mesh.h -- iso-surface extraction on the device (included by lab4d_hip.h).  SURVEY.md 8f row 3.
 *
 * Replaces (paths relative to lab4d/):
 *   utils/geom_utils.py:442-503   marching_cubes: skimage.measure.marching_cubes(volume, level, spacing, mask) on the host,
 *                                 trimesh.Trimesh(...).split() + "keep the component with the most vertices"
 *
 * Volume: (Gx, Gy, Gz) fp32, Gz fastest (the layout of torch.cartesian_prod / geom_utils.sample_grid), Gx, Gy, Gz >= 1 and
 * Gx * Gy * Gz < 2^31 / 3; mask: uint8 of the same shape or NULL.  Not assumed cubic or a power of two.
 *
 * Defined behaviour:
 *   - a value is inside iff value < level (NaN: outside).  A cell is meshed iff all 8 corners have mask != 0 and finite values; every
 *     other cell is skipped.  Triangles of a cell come from the generated case table lab4d_amd/csrc/mc_tables.hpp.
 *   - every grid point owns its +i, +j, +k edges.  A vertex exists for an owned edge iff the edge is crossed and at least one of the
 *     (up to four) cells around it is meshed.  Vertices are numbered by ascending (linear index of the owner) * 3 + axis.
 *   - faces are numbered by ascending linear cell index, then table order inside the cell; int32 vertex indices; the normal
 *     (v1 - v0) x (v2 - v0) points towards increasing values.
 *   - no atomics on the extraction path (count -> exclusive scan -> write), so the output is bit-reproducible.
 * Output sizes depend on the data, hence two phases: lab4d_mesh_count leaves {n_verts, n_faces} on the device, the caller reads
 * them back ONCE, allocates, and calls lab4d_mesh_emit with the same volume, level and work buffer.  Not capturable in a hipGraph.
 */
#ifndef LAB4D_MESH_H
#define LAB4D_MESH_H

/* int32 words of work space that count / emit need for this volume (host-only; -1 for an invalid shape) */
int64_t lab4d_mesh_work_ints(int Gx, int Gy, int Gz);

/* Phase 1: classifies cells and edges into `work`, counts[0] = n_verts, counts[1] = n_faces (device int32[2]). */
int lab4d_mesh_count(const float* sdf, const unsigned char* mask, int Gx, int Gy, int Gz, float level, int32_t* work, int32_t* counts,
                     void* stream);

/* Phase 2: verts (n_verts, 3) fp32 and faces (n_faces, 3) int32, n_verts / n_faces as read back from `counts` (nothing is written
 * beyond them).  xform: device float[6] = origin xyz, step xyz (vertex = origin + step * index position), or NULL for index space.
 * `work` must be untouched since lab4d_mesh_count on the same sdf / level. */
int lab4d_mesh_emit(const float* sdf, int Gx, int Gy, int Gz, float level, const float* xform, int32_t* work, int n_verts, int n_faces,
                    float* verts, int32_t* faces, void* stream);

/* int32 words of work space of lab4d_mesh_largest_component (host-only; -1 for negative sizes) */
int64_t lab4d_mesh_component_work_ints(int n_verts, int n_faces);

/* Keeps the largest connected component (geom_utils.py:497-501).  Connectivity: vertices joined by a face; size: VERTEX count; ties: the
 * component that holds the smallest vertex index.  Survivors keep their order, faces are re-indexed.  out_verts / out_faces are sized
 * like the inputs; out_counts[0] = vertices kept, out_counts[1] = faces kept (device int32[2]).  Labels are propagated by atomicMin
 * hooking + pointer jumping until a pass changes nothing; the call synchronises the stream to look at that flag every few passes.
 * stats (host int[2], may be NULL): number of label passes run, number of host read-backs. */
int lab4d_mesh_largest_component(const float* verts, const int32_t* faces, int n_verts, int n_faces, int32_t* work, float* out_verts,
                                 int32_t* out_faces, int32_t* out_counts, int* stats, void* stream);

#endif /* LAB4D_MESH_H */
