// Per-cell / per-edge arithmetic of the iso-surface extractor (csrc/mesh.hip; contract: include/lab4d_mesh.h) -- what the reference does
// with skimage.measure.marching_cubes in geom_utils.marching_cubes (lab4d/utils/geom_utils.py:442-503).
// Plain C++ behind LAB4D_HD (see hd_math.hpp): the kernels run it one thread per grid point, tests/host_harness/mesh_host.cpp compiles
// it with g++ (-ffp-contract=off) as a serial loop over the same functions and the same table (mc_tables.hpp), so that the CPU test-suite
// can pin the mesh by its properties and the GPU suite can hold the kernels bit for bit to the CPU twin.
//
// Defined behaviour (ours; INTEGRATION.md "Proxy mesh on the device"):
//   * a grid value is INSIDE iff value < level; a comparison with NaN is false, so NaN counts as outside;
//   * a cell is MESHED iff all 8 of its corners have mask != 0 (no mask: all set) and all 8 values are finite.  Any other cell is skipped:
//     it contributes no triangle, and no vertex is ever interpolated from an inf / NaN value;
//   * the vertex on a crossed edge from grid point p (value a) to p + e_axis (value b) sits at index-space coordinate
//     p[axis] + (level - a) / (b - a); a != b is guaranteed by the crossing.  World position = origin + step * index position, per axis,
//     product and sum rounded separately (no fused multiply-add on either side).
#pragma once
#include "hd_math.hpp"
#include "mc_tables.hpp"

namespace lab4d_mc {
using lab4d_rn::add_rn;
using lab4d_rn::div_rn;
using lab4d_rn::finite_f;
using lab4d_rn::mul_rn;

LAB4D_HD bool inside(float v, float level) { return v < level; }

// corner c of the cell whose corner 0 has linear index 0 in a (Gx, Gy, Gz) volume, Gz fastest
LAB4D_HD long corner_offset(int c, int Gy, int Gz) { return (long)((c >> 0) & 1) * Gy * Gz + (long)((c >> 1) & 1) * Gz + ((c >> 2) & 1); }

// v[8], m[8] (m may be null): corner values / mask bytes in corner order
LAB4D_HD bool cell_meshed(const float* v, const unsigned char* m) {
  bool ok = true;
  for (int c = 0; c < 8; ++c) ok = ok && finite_f(v[c]) && (m == nullptr || m[c] != 0);
  return ok;
}

LAB4D_HD int cell_case(const float* v, float level) {
  int idx = 0;
  for (int c = 0; c < 8; ++c) idx |= inside(v[c], level) ? (1 << c) : 0;
  return idx;
}

LAB4D_HD bool edge_crossed(float a, float b, float level) { return inside(a, level) != inside(b, level); }

// index-space coordinate along `axis` of the vertex on the crossed edge that starts at integer coordinate p (values a at p, b at p + 1)
LAB4D_HD float edge_vertex(int p, float a, float b, float level) { return add_rn((float)p, div_rn(level - a, b - a)); }

LAB4D_HD float to_world(float index_pos, float origin, float step) { return add_rn(origin, mul_rn(step, index_pos)); }

}  // namespace lab4d_mc
