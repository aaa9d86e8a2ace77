// CPU twin of lab4d_amd/csrc/meshray.hip: serial loops over the SAME functions (csrc/meshray_math.hpp) with the layout and the argument checks
// of include/lab4d_meshray.h.  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_meshray_host.py holds it to numpy float64.
// Returns -1 for arguments outside the contract.  A folder of its own: the census of tests/test_host_twin.py counts the twins beside it.
#include <stdint.h>

#include "meshray_math.hpp"

namespace mr = lab4d_mray;

// Packs the faces into tris (12 * n_faces floats, 16-byte aligned) and builds the lists: cell_start (G^3 + 1) is always written; cell_list
// (ascending face index within a cell) only when it is not NULL.  Returns the length of the list: call once with cell_list == NULL to size it.
extern "C" int meshray_host_build(const float* verts, const int32_t* faces, int n_verts, int n_faces, const float* aabb, int G, float* tris,
                                  int32_t* cell_start, int32_t* cell_list) {
  if (G < 1 || G > mr::kMaxG || n_verts < 0 || n_faces < 0 || n_faces > 2147483647 / mr::kTriFloats) return -1;
  const long n_cells = (long)G * G * G;
  mr::Quad* rec = (mr::Quad*)tris;
  for (long c = 0; c <= n_cells; ++c) cell_start[c] = 0;
  for (int pass = 0; pass < 2; ++pass) {  // 0: count into cell_start[c + 1], then the prefix sum; 1: fill
    for (long f = 0; f < n_faces; ++f) {
      if (pass == 0) mr::pack_face(verts, faces, n_verts, f, rec + 3 * f);
      int i0[3], i1[3];
      if (!mr::face_cells(rec + 3 * f, aabb, G, i0, i1)) continue;
      for (int z = i0[2]; z <= i1[2]; ++z)
        for (int y = i0[1]; y <= i1[1]; ++y)
          for (int x = i0[0]; x <= i1[0]; ++x) {
            const long c = x + (long)G * (y + (long)G * z);
            if (pass == 0) ++cell_start[c + 1];
            else cell_list[cell_start[c]++] = (int32_t)f;  // (cell_start[c] runs up to the start of c + 1: shifted back below)
          }
    }
    if (pass == 0) {
      for (long c = 0; c < n_cells; ++c) cell_start[c + 1] += cell_start[c];
      if (!cell_list) break;
    } else {
      for (long c = n_cells; c > 0; --c) cell_start[c] = cell_start[c - 1];
      cell_start[0] = 0;
    }
  }
  return cell_start[n_cells];
}

extern "C" int meshray_host_cast(const float* origin, const float* dir, const float* t_range, long R, const float* tris, int n_faces, const float* aabb, int G,
                                 const int32_t* cell_start, const int32_t* cell_list, float* t, int32_t* face, float* u, float* v, int32_t* front,
                                 int32_t* n_tests) {
  if (R < 0 || G < 1 || G > mr::kMaxG || n_faces < 0 || n_faces > 2147483647 / mr::kTriFloats) return -1;
  for (long r = 0; r < R; ++r) {
    const mr::Hit h = mr::cast_ray(origin + 3 * r, dir + 3 * r, t_range[2 * r], t_range[2 * r + 1], aabb, G, tris, n_faces, cell_start, cell_list);
    t[r] = h.t, face[r] = h.face, u[r] = h.u, v[r] = h.v, front[r] = h.front, n_tests[r] = h.n_tests;
  }
  return 0;
}

// REJECT and CLIP alone: code (R) = 0 rejected / 1 empty clip / 2 clipped, t_clip (R,2) = {t_enter, t_exit} (t0, t0 unless the code is 2)
extern "C" void meshray_host_clip(const float* origin, const float* dir, const float* t_range, const float* aabb, long R, float* t_clip, int32_t* code) {
  for (long r = 0; r < R; ++r) {
    t_clip[2 * r] = t_clip[2 * r + 1] = t_range[2 * r];
    code[r] = mr::clip_ray(origin + 3 * r, dir + 3 * r, t_range[2 * r], t_range[2 * r + 1], aabb, t_clip + 2 * r, t_clip + 2 * r + 1);
  }
}
