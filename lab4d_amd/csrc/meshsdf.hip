// Signed distance from points to a triangle mesh, brute force: every point against every face.  Contract: include/lab4d_meshsdf.h; every
// rule and all of the arithmetic: meshsdf_math.hpp, shared with the CPU twin tests/host_harness/meshsdf_host.cpp, to which the distance,
// the face index and the closest point are held bit for bit.  No atomics, no read-back, no allocation: the call can be captured in a
// hipGraph.
#include "common.hpp"
#include "meshsdf_math.hpp"

namespace lab4d {
namespace msdf = lab4d_msdf;

constexpr int kSdfBlock = 256;  // points per block (4 waves), and faces per LDS tile; a face in LDS: {a xyz, valid}, {b xyz, -}, {c xyz, -}

// Grid (ceil(n_pts / 256), n_slices).  One point per lane, in registers; the block walks the faces of its slice in tiles of 256.  A tile
// is gathered cooperatively (lane t: face t of the tile -- indices, nine coordinates, the VALID test) into LDS; then every lane reads the
// same LDS address at the same time (a broadcast: no bank conflict) while it walks the tile.  work == nullptr (n_slices == 1): the final
// outputs are written here; otherwise the slice's partial result goes to work[(slice * 6 + k) * n_pts + i].
__global__ void __launch_bounds__(kSdfBlock) k_mesh_sdf_partial(const float* __restrict__ verts, const int32_t* __restrict__ faces, int n_verts, int n_faces,
                                                                 const float* __restrict__ pts, long n_pts, int n_slices, float* __restrict__ work,
                                                                 float* __restrict__ sdf, int32_t* __restrict__ face_idx, float* __restrict__ closest) {
  __shared__ float4 tile[kSdfBlock * 3];
  const long i = (long)blockIdx.x * kSdfBlock + threadIdx.x;
  const bool live = i < n_pts;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (live) px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
  const bool pt_ok = msdf::point_finite(px, py, pz);
  msdf::Best r = msdf::best_init(px, py, pz);
  const int s = blockIdx.y;
  const long lo = msdf::slice_lo(s, n_faces, n_slices), hi = msdf::slice_lo(s + 1, n_faces, n_slices);
  for (long t0 = lo; t0 < hi; t0 += kSdfBlock) {
    const long f = t0 + threadIdx.x;
    const int n_tile = (int)(hi - t0 < kSdfBlock ? hi - t0 : kSdfBlock);
    if (f < hi) {
      float v[9];
      const bool ok = msdf::load_tri(verts, faces, n_verts, f, v);
      tile[3 * threadIdx.x] = make_float4(v[0], v[1], v[2], ok ? 1.f : 0.f);
      tile[3 * threadIdx.x + 1] = make_float4(v[3], v[4], v[5], 0.f);
      tile[3 * threadIdx.x + 2] = make_float4(v[6], v[7], v[8], 0.f);
    }
    __syncthreads();
    if (pt_ok) {  // (uniform per wave only by accident; the barrier stays outside)
      for (int j = 0; j < n_tile; ++j) {
        const float4 a = tile[3 * j], b = tile[3 * j + 1], c = tile[3 * j + 2];
        if (a.w != 0.f) {
          const float v[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
          msdf::best_visit(r, px, py, pz, v, (int32_t)(t0 + j));
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
  if (work == nullptr) {
    sdf[i] = msdf::best_sdf(r, pt_ok);
    if (face_idx) face_idx[i] = r.face;
    if (closest) closest[3 * i] = r.qx, closest[3 * i + 1] = r.qy, closest[3 * i + 2] = r.qz;
    return;
  }
  float* w = work + (long)s * msdf::kWorkWords * n_pts + i;
  w[0] = r.d2;
  w[n_pts] = __int_as_float(r.face);
  w[2 * n_pts] = r.qx;
  w[3 * n_pts] = r.qy;
  w[4 * n_pts] = r.qz;
  w[5 * n_pts] = r.wsum;
}

// One lane per point: the slices' partial results folded in ascending order.
__global__ void __launch_bounds__(kSdfBlock) k_mesh_sdf_reduce(const float* __restrict__ work, const float* __restrict__ pts, long n_pts, int n_slices,
                                                                float* __restrict__ sdf, int32_t* __restrict__ face_idx, float* __restrict__ closest) {
  const long i = (long)blockIdx.x * kSdfBlock + threadIdx.x;
  if (i >= n_pts) return;
  const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
  msdf::Best r = msdf::best_init(px, py, pz);
  for (int s = 0; s < n_slices; ++s) {
    const float* w = work + (long)s * msdf::kWorkWords * n_pts + i;
    const msdf::Best part{w[0], w[2 * n_pts], w[3 * n_pts], w[4 * n_pts], w[5 * n_pts], __float_as_int(w[n_pts])};
    msdf::best_merge(r, part);
  }
  sdf[i] = msdf::best_sdf(r, msdf::point_finite(px, py, pz));
  if (face_idx) face_idx[i] = r.face;
  if (closest) closest[3 * i] = r.qx, closest[3 * i + 1] = r.qy, closest[3 * i + 2] = r.qz;
}

}  // namespace lab4d
using namespace lab4d;

extern "C" int lab4d_mesh_sdf(const float* verts, const int32_t* faces, int n_verts, int n_faces, const float* pts, long n_pts, int n_slices, float* work,
                              float* sdf, int32_t* face_idx, float* closest, void* stream) {
  LAB4D_REQUIRE(n_verts >= 0 && n_faces >= 0 && n_pts >= 0, "mesh_sdf: negative size (n_verts %d, n_faces %d, n_pts %ld)", n_verts, n_faces, n_pts);
  LAB4D_REQUIRE(n_slices >= 1 && n_slices <= 65535, "mesh_sdf: n_slices = %d outside [1, 65535]", n_slices);
  LAB4D_REQUIRE(n_faces <= 2147483647 / 3, "mesh_sdf: n_faces = %d, must be below 2^31 / 3", n_faces);
  LAB4D_REQUIRE(n_pts < (1L << 31), "mesh_sdf: n_pts = %ld, must be below 2^31: query the points in chunks", n_pts);
  LAB4D_REQUIRE(n_slices == 1 || (long)n_slices * lab4d_msdf::kWorkWords <= (2147483647L / (n_pts > 0 ? n_pts : 1)),
                "mesh_sdf: n_slices * n_pts * 6 = %d * %ld * 6 work words reach 2^31: query the points in chunks", n_slices, n_pts);
  if (n_pts == 0) return LAB4D_OK;
  LAB4D_REQUIRE(pts && sdf, "mesh_sdf: null pointer (pts, sdf)");
  LAB4D_REQUIRE(n_faces == 0 || faces, "mesh_sdf: null pointer (faces)");
  LAB4D_REQUIRE(n_faces == 0 || n_verts == 0 || verts, "mesh_sdf: null pointer (verts)");
  LAB4D_REQUIRE(n_slices == 1 || work, "mesh_sdf: null pointer (work) with n_slices = %d", n_slices);
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n_pts + kSdfBlock - 1) / kSdfBlock);
  float* part = n_slices == 1 ? nullptr : work;
  hipLaunchKernelGGL(k_mesh_sdf_partial, dim3(blocks, (unsigned)n_slices), dim3(kSdfBlock), 0, st, verts, faces, n_verts, n_faces, pts, n_pts, n_slices, part,
                     sdf, face_idx, closest);
  if (int e = check_launch("mesh_sdf (partial)")) return e;
  if (n_slices > 1) {
    hipLaunchKernelGGL(k_mesh_sdf_reduce, dim3(blocks), dim3(kSdfBlock), 0, st, (const float*)work, pts, n_pts, n_slices, sdf, face_idx, closest);
    return check_launch("mesh_sdf (reduce)");
  }
  return LAB4D_OK;
}
