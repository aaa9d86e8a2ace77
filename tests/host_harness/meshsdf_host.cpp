// CPU twin of lab4d_amd/csrc/meshsdf.hip: serial loops over the SAME functions (csrc/meshsdf_math.hpp) with the layout of
// include/lab4d_meshsdf.h.  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_meshsdf_host.py pins it against numpy
// in float64, the GPU suite holds the kernels' distance, face and closest point bit for bit to it (tests/test_gpu_zzzzzzmeshsdf.py).
#include <stdint.h>

#include "meshsdf_math.hpp"

namespace msdf = lab4d_msdf;

// the faces [lo, hi) in ascending order, as one block of the kernel walks its slice
static msdf::Best walk(const float* verts, const int32_t* faces, int n_verts, long lo, long hi, const float* p) {
  msdf::Best r = msdf::best_init(p[0], p[1], p[2]);
  if (!msdf::point_finite(p[0], p[1], p[2])) return r;
  for (long f = lo; f < hi; ++f) {
    float v[9];
    if (msdf::load_tri(verts, faces, n_verts, f, v)) msdf::best_visit(r, p[0], p[1], p[2], v, (int32_t)f);
  }
  return r;
}

static void store(const msdf::Best& r, const float* p, long i, float* sdf, float* d2, float* wsum, int32_t* face_idx, float* closest) {
  sdf[i] = msdf::best_sdf(r, msdf::point_finite(p[0], p[1], p[2]));
  if (d2) d2[i] = r.d2;
  if (wsum) wsum[i] = r.wsum;
  if (face_idx) face_idx[i] = r.face;
  if (closest) closest[3 * i] = r.qx, closest[3 * i + 1] = r.qy, closest[3 * i + 2] = r.qz;
}

// The whole query.  d2 (n_pts: the winner's squared distance, +inf without one), wsum (n_pts: the sum of the atan2 terms, w = wsum / 2 pi),
// face_idx and closest may be null.
extern "C" void meshsdf_host_query(const float* verts, const int32_t* faces, int n_verts, int n_faces, const float* pts, long n_pts, float* sdf,
                                   float* d2, float* wsum, int32_t* face_idx, float* closest) {
  for (long i = 0; i < n_pts; ++i) store(walk(verts, faces, n_verts, 0, n_faces, pts + 3 * i), pts + 3 * i, i, sdf, d2, wsum, face_idx, closest);
}

// The order of k_mesh_sdf_partial + k_mesh_sdf_reduce: every slice on its own, then the slices folded in ascending order.
extern "C" void meshsdf_host_query_sliced(const float* verts, const int32_t* faces, int n_verts, int n_faces, const float* pts, long n_pts, int n_slices,
                                          float* sdf, float* d2, float* wsum, int32_t* face_idx, float* closest) {
  for (long i = 0; i < n_pts; ++i) {
    const float* p = pts + 3 * i;
    msdf::Best r = msdf::best_init(p[0], p[1], p[2]);
    for (int s = 0; s < n_slices; ++s)
      msdf::best_merge(r, walk(verts, faces, n_verts, msdf::slice_lo(s, n_faces, n_slices), msdf::slice_lo(s + 1, n_faces, n_slices), p));
    store(r, p, i, sdf, d2, wsum, face_idx, closest);
  }
}

// the faces' VALID flags (n_faces) uint8
extern "C" void meshsdf_host_valid(const float* verts, const int32_t* faces, int n_verts, int n_faces, uint8_t* valid) {
  for (long f = 0; f < n_faces; ++f) {
    float v[9];
    valid[f] = msdf::load_tri(verts, faces, n_verts, f, v) ? 1 : 0;
  }
}
