// CPU twin of lab4d_amd/csrc/mesh.hip: a serial loop over grid points using the SAME per-cell functions (csrc/mesh_math.hpp) and the SAME
// case table (csrc/mc_tables.hpp), with the ordering contract of include/lab4d_mesh.h.  Built by tests/host_twin.py with
// g++ -ffp-contract=off; the GPU suite holds the kernels bit for bit to it (tests/test_gpu_zzzmesh.py).
#include <stdint.h>

#include <vector>

#include "mesh_math.hpp"

namespace mc = lab4d_mc;

// counts[0] = n_verts, counts[1] = n_faces; verts / faces are written up to cap_verts / cap_faces rows (call with 0 / 0 to count first).
// xform: origin xyz, step xyz, or null for index space.
extern "C" void mesh_host_extract(const float* sdf, const unsigned char* mask, int Gx, int Gy, int Gz, float level, const float* xform, float* verts,
                                  int32_t* faces, long cap_verts, long cap_faces, int32_t* counts) {
  const long n = (long)Gx * Gy * Gz;
  const int G[3] = {Gx, Gy, Gz};
  const long stride[3] = {(long)Gy * Gz, (long)Gz, 1};
  std::vector<unsigned char> cases(n, 0);
  for (long lin = 0; lin < n; ++lin) {
    const int k = (int)(lin % Gz), j = (int)((lin / Gz) % Gy), i = (int)(lin / ((long)Gz * Gy));
    if (!(i + 1 < Gx && j + 1 < Gy && k + 1 < Gz)) continue;
    float v[8];
    unsigned char m[8];
    for (int c = 0; c < 8; ++c) {
      const long o = lin + mc::corner_offset(c, Gy, Gz);
      v[c] = sdf[o];
      m[c] = mask ? mask[o] : (unsigned char)1;
    }
    if (mc::cell_meshed(v, m)) cases[lin] = (unsigned char)mc::cell_case(v, level);
  }
  std::vector<int32_t> edge_id(3 * n, -1);
  long nv = 0;
  for (long lin = 0; lin < n; ++lin) {
    const int p[3] = {(int)(lin / ((long)Gz * Gy)), (int)((lin / Gz) % Gy), (int)(lin % Gz)};
    for (int a = 0; a < 3; ++a) {
      if (p[a] + 1 >= G[a]) continue;
      const float v0 = sdf[lin], v1 = sdf[lin + stride[a]];
      if (!mc::edge_crossed(v0, v1, level)) continue;
      const int b = (a + 1) % 3, c = (a + 2) % 3;
      bool any = false;
      for (int q = 0; q < 4; ++q) {
        const int db = q & 1, dc = q >> 1;
        if (p[b] - db < 0 || p[c] - dc < 0) continue;
        any = any || cases[lin - db * stride[b] - dc * stride[c]] != 0;
      }
      if (!any) continue;
      edge_id[lin * 3 + a] = (int32_t)nv;
      if (nv < cap_verts) {
        float q[3] = {(float)p[0], (float)p[1], (float)p[2]};
        q[a] = mc::edge_vertex(p[a], v0, v1, level);
        for (int d = 0; d < 3; ++d) verts[nv * 3 + d] = xform ? mc::to_world(q[d], xform[d], xform[3 + d]) : q[d];
      }
      ++nv;
    }
  }
  long nf = 0;
  for (long lin = 0; lin < n; ++lin) {
    const int cs = cases[lin];
    for (int t = 0; t < mc::kTriCount[cs]; ++t) {
      if (nf < cap_faces)
        for (int m = 0; m < 3; ++m) {
          const int e = mc::kTriEdges[cs][3 * t + m];
          faces[nf * 3 + m] = edge_id[(lin + mc::corner_offset(mc::kEdgeCorner[e], Gy, Gz)) * 3 + mc::kEdgeAxis[e]];
        }
      ++nf;
    }
  }
  counts[0] = (int32_t)nv;
  counts[1] = (int32_t)nf;
}

static int find_root(std::vector<int32_t>& parent, int v) {
  while (parent[v] != v) {
    parent[v] = parent[parent[v]];
    v = parent[v];
  }
  return v;
}

// include/lab4d_mesh.h lab4d_mesh_largest_component: vertices joined by a face; size = vertex count; ties to the component holding the
// smallest vertex index; survivors keep their order.  out_* sized like the inputs.
extern "C" void mesh_host_largest_component(const float* verts, const int32_t* faces, int n_verts, int n_faces, float* out_verts, int32_t* out_faces,
                                            int32_t* counts) {
  std::vector<int32_t> parent(n_verts), size(n_verts, 0), remap(n_verts, -1);
  for (int v = 0; v < n_verts; ++v) parent[v] = v;
  for (long f = 0; f < n_faces; ++f)
    for (int m = 1; m < 3; ++m) {
      const int a = find_root(parent, faces[f * 3]), b = find_root(parent, faces[f * 3 + m]);
      if (a != b) parent[a > b ? a : b] = a > b ? b : a;  // the smaller index stays root: root = smallest vertex of the component
    }
  for (int v = 0; v < n_verts; ++v) ++size[find_root(parent, v)];
  int win = -1;
  for (int v = 0; v < n_verts; ++v)
    if (parent[v] == v && (win < 0 || size[v] > size[win])) win = v;
  int nv = 0, nf = 0;
  for (int v = 0; v < n_verts; ++v)
    if (find_root(parent, v) == win) {
      for (int d = 0; d < 3; ++d) out_verts[(long)nv * 3 + d] = verts[(long)v * 3 + d];
      remap[v] = nv++;
    }
  for (long f = 0; f < n_faces; ++f)
    if (find_root(parent, faces[f * 3]) == win) {
      for (int m = 0; m < 3; ++m) out_faces[(long)nf * 3 + m] = remap[faces[f * 3 + m]];
      ++nf;
    }
  counts[0] = nv;
  counts[1] = nf;
}
