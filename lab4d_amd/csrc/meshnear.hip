// Closest point and signed distance from points to a triangle mesh through the face grid of meshray.hip.  Contract: include/lab4d_meshnear.h;
// every rule and all of the arithmetic: meshnear_math.hpp, shared with the CPU twin tests/host_harness/meshnear/meshnear_host.cpp, to which d2,
// face, closest, region and n_tests are held bit for bit, and sdf wherever the region is a face or an edge.  No atomics, no read-back and no
// allocation: capturable in a hipGraph.
#include "common.hpp"
#include "meshnear_math.hpp"

namespace lab4d {
namespace mn = lab4d_mnear;

// One lane per point, grid-stride.  A lane keeps the point (3), the best d2, q, face and region (6), its start cell, the shell and the three
// loop indices (7) and the count; a face test is three 16-byte loads.  A lane leaves the walk when its stop rule holds; the wave runs on until its
// last lane has, then the sign pass (edge and vertex regions only) reads the list of q's cell.
__global__ void __launch_bounds__(mn::kBlock) k_mesh_closest(const float* __restrict__ pts, long N, const float* __restrict__ tris, int n_faces,
                                                              const float* __restrict__ aabb_, int G, const int32_t* __restrict__ cell_start,
                                                              const int32_t* __restrict__ cell_list, int sign_mode, int orient, float* __restrict__ sdf,
                                                              float* __restrict__ d2, int32_t* __restrict__ face, float* __restrict__ closest,
                                                              int32_t* __restrict__ region, int32_t* __restrict__ n_tests) {
  const float aabb[6] = {aabb_[0], aabb_[1], aabb_[2], aabb_[3], aabb_[4], aabb_[5]};
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)N; i += gridDim.x * blockDim.x) {  // (N < 2^31, the stride <= 2^19: no wrap)
    const mn::Found r = mn::find_nearest(pts[3 * (long)i], pts[3 * (long)i + 1], pts[3 * (long)i + 2], aabb, G, tris, n_faces, cell_start, cell_list, sign_mode, orient);
    sdf[i] = r.sdf;
    if (d2) d2[i] = r.d2;
    if (face) face[i] = r.face;
    if (closest) closest[3 * (long)i] = r.qx, closest[3 * (long)i + 1] = r.qy, closest[3 * (long)i + 2] = r.qz;
    if (region) region[i] = r.region;
    if (n_tests) n_tests[i] = r.n_tests;
  }
}

}  // namespace lab4d
using namespace lab4d;

extern "C" int lab4d_mesh_closest(const float* pts, long N, const float* tris, int n_faces, const float* aabb, int G, const int32_t* cell_start,
                                  const int32_t* cell_list, int sign_mode, int orient, float* sdf, float* d2, int32_t* face, float* closest,
                                  int32_t* region, int32_t* n_tests, void* stream) {
  LAB4D_REQUIRE(N >= 0 && N < (1L << 31), "mesh_closest: N = %ld outside [0, 2^31)", N);
  LAB4D_REQUIRE(G >= 1 && G <= lab4d_mray::kMaxG, "mesh_closest: G = %d outside [1, %d]", G, lab4d_mray::kMaxG);
  LAB4D_REQUIRE(n_faces >= 0 && n_faces <= 2147483647 / lab4d_mray::kTriFloats, "mesh_closest: n_faces = %d outside [0, 2^31 / 12]", n_faces);
  LAB4D_REQUIRE(sign_mode == 0 || sign_mode == 1, "mesh_closest: sign_mode = %d is neither 0 (unsigned) nor 1 (pseudonormal)", sign_mode);
  LAB4D_REQUIRE(orient == 1 || orient == -1, "mesh_closest: orient = %d is neither +1 nor -1", orient);
  LAB4D_REQUIRE(aabb, "mesh_closest: null pointer (aabb)");
  LAB4D_REQUIRE(n_faces == 0 || (tris && cell_start), "mesh_closest: null pointer (tris, cell_start)");
  if (N == 0) return LAB4D_OK;  // (the per-point arrays are empty: an empty tensor's pointer is NULL)
  LAB4D_REQUIRE(pts && sdf, "mesh_closest: null pointer (pts, sdf)");
  hipLaunchKernelGGL(k_mesh_closest, dim3(grid_1d(N, mn::kBlock, 2048)), dim3(mn::kBlock), 0, (hipStream_t)stream, pts, N, tris, n_faces, aabb, G, cell_start,
                     cell_list, sign_mode, orient, sdf, d2, face, closest, region, n_tests);
  return check_launch("mesh_closest");
}
