// CPU twin of lab4d_amd/csrc/meshnear.hip: a serial loop over the SAME function (csrc/meshnear_math.hpp) with the layout and the argument checks
// of include/lab4d_meshnear.h.  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_meshnear_host.py holds it to the brute-force
// twin (meshsdf_host.cpp) word for word and its sign to float64.  The grid's lists come from the ray caster's twin (meshray/meshray_host.cpp).
// Returns -1 for arguments outside the contract.  A folder of its own: the census of tests/test_host_twin.py counts the twins beside it.
#include <stdint.h>

#include "meshnear_math.hpp"

namespace mn = lab4d_mnear;

// n_cells (may be NULL): the cells each point's walk visited -- the twin's own extra, for measurement
extern "C" int meshnear_host_closest(const float* pts, long N, const float* tris, int n_faces, const float* aabb, int G, const int32_t* cell_start,
                                     const int32_t* cell_list, int sign_mode, int orient, float* sdf, float* d2, int32_t* face, float* closest,
                                     int32_t* region, int32_t* n_tests, int32_t* n_cells) {
  if (N < 0 || N >= (1L << 31) || G < 1 || G > lab4d_mray::kMaxG || n_faces < 0 || n_faces > 2147483647 / lab4d_mray::kTriFloats) return -1;
  if ((sign_mode != 0 && sign_mode != 1) || (orient != 1 && orient != -1) || !aabb || (n_faces && !(tris && cell_start))) return -1;
  if (N == 0) return 0;
  if (!pts || !sdf) return -1;
  for (long i = 0; i < N; ++i) {
    const mn::Found r = mn::find_nearest(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], aabb, G, tris, n_faces, cell_start, cell_list, sign_mode, orient);
    sdf[i] = r.sdf;
    if (d2) d2[i] = r.d2;
    if (face) face[i] = r.face;
    if (closest) closest[3 * i] = r.qx, closest[3 * i + 1] = r.qy, closest[3 * i + 2] = r.qz;
    if (region) region[i] = r.region;
    if (n_tests) n_tests[i] = r.n_tests;
    if (n_cells) n_cells[i] = r.n_cells;
  }
  return 0;
}

// closest_reg and msdf::closest_d2 side by side on n (point, triangle) pairs: tri (n,9) = a, b, c; out_new, out_old (n,4) = d2, q
extern "C" void meshnear_host_restated(const float* pts, const float* tri, long n, float* out_new, int32_t* region, float* out_old) {
  for (long i = 0; i < n; ++i) {
    const float* p = pts + 3 * i;
    const float* t = tri + 9 * i;
    out_new[4 * i] = mn::closest_reg(p[0], p[1], p[2], t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], out_new[4 * i + 1], out_new[4 * i + 2],
                                     out_new[4 * i + 3], region[i]);
    out_old[4 * i] = lab4d_msdf::closest_d2(p[0], p[1], p[2], t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], out_old[4 * i + 1], out_old[4 * i + 2],
                                            out_old[4 * i + 3]);
  }
}
