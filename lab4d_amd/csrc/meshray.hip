// Ray casting against a triangle mesh through a uniform face grid.  Contract: include/lab4d_meshray.h; every rule and all of the arithmetic:
// meshray_math.hpp, shared with the CPU twin tests/host_harness/meshray/meshray_host.cpp, to which the cast's t, face, u, v and front are
// held bit for bit and the cell lists after sorting.  The build counts with integer atomics (deterministic totals), scans, and fills with
// integer atomics (the order within a cell is unspecified: FIRST HIT does not depend on it).  The cast has no atomics, no read-back and no
// allocation: capturable in a hipGraph.
#include "common.hpp"
#include "meshray_math.hpp"

namespace lab4d {
namespace mr = lab4d_mray;

// One lane per face: packs the face (three 16-byte words) and counts it into every cell of its padded index box.
__global__ void __launch_bounds__(mr::kBlock) k_meshgrid_count(const float* __restrict__ verts, const int32_t* __restrict__ faces, int n_verts, int n_faces,
                                                                const float* __restrict__ aabb_, int G, mr::Quad* __restrict__ tris,
                                                                int32_t* __restrict__ cell_count) {
  const float aabb[6] = {aabb_[0], aabb_[1], aabb_[2], aabb_[3], aabb_[4], aabb_[5]};
  for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += (long)gridDim.x * blockDim.x) {
    mr::Quad rec[3];
    mr::pack_face(verts, faces, n_verts, f, rec);
    tris[3 * f] = rec[0], tris[3 * f + 1] = rec[1], tris[3 * f + 2] = rec[2];
    int i0[3], i1[3];
    if (!mr::face_cells(rec, aabb, G, i0, i1)) continue;
    for (int z = i0[2]; z <= i1[2]; ++z)
      for (int y = i0[1]; y <= i1[1]; ++y)
        for (int x = i0[0]; x <= i1[0]; ++x) atomicAdd(&cell_count[x + G * (y + G * z)], 1);
  }
}

// One lane per face: the packing alone (the vertices moved, the lists stay).
__global__ void __launch_bounds__(mr::kBlock) k_meshgrid_pack(const float* __restrict__ verts, const int32_t* __restrict__ faces, int n_verts, int n_faces,
                                                               mr::Quad* __restrict__ tris) {
  for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += (long)gridDim.x * blockDim.x) {
    mr::Quad rec[3];
    mr::pack_face(verts, faces, n_verts, f, rec);
    tris[3 * f] = rec[0], tris[3 * f + 1] = rec[1], tris[3 * f + 2] = rec[2];
  }
}

// The exclusive scan of the cell counts, in the pattern of compact.hip: sums of blocks of 1,024 cells, one workgroup scans those, every block
// scans its own cells on top of its offset.  cell_start[n_cells] = *total = the length of the list.
__global__ void __launch_bounds__(256) k_meshgrid_block_sums(const int32_t* __restrict__ cell_count, int n_cells, int32_t* __restrict__ block_sum) {
  __shared__ int w[4];
  const int base = blockIdx.x * mr::kScanBlock + threadIdx.x * 4;
  int s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (base + i < n_cells) s += cell_count[base + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) block_sum[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}

__global__ void __launch_bounds__(1024) k_meshgrid_scan_blocks(int32_t* __restrict__ block_sum, int nblocks, int32_t* __restrict__ cell_start_end,
                                                                int32_t* __restrict__ total) {
  __shared__ int part[1024];
  const int per = (nblocks + 1023) / 1024;
  const int b0 = threadIdx.x * per;
  int s = 0;
  for (int i = 0; i < per; ++i)
    if (b0 + i < nblocks) s += block_sum[b0 + i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (int i = 0; i < per; ++i)
    if (b0 + i < nblocks) {
      const int c = block_sum[b0 + i];
      block_sum[b0 + i] = run;
      run += c;
    }
  if (threadIdx.x == 1023) *cell_start_end = part[1023], *total = part[1023];
}

__global__ void __launch_bounds__(256) k_meshgrid_offsets(const int32_t* __restrict__ cell_count, int n_cells, const int32_t* __restrict__ block_offset,
                                                           int32_t* __restrict__ cell_start) {
  __shared__ int part[256];
  const int base = blockIdx.x * mr::kScanBlock + threadIdx.x * 4;
  int c[4], s = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = base + i < n_cells ? cell_count[base + i] : 0, s += c[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = block_offset[blockIdx.x] + (threadIdx.x ? part[threadIdx.x - 1] : 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (base + i < n_cells) cell_start[base + i] = run;
    run += c[i];
  }
}

// One lane per face: a slot of every cell of its index box, claimed with an integer atomic on the cell's cursor (zeroed by the entry point).
// A slot at or behind n_list (the buffers changed between the count and the fill) is not written.
__global__ void __launch_bounds__(mr::kBlock) k_meshgrid_fill(const mr::Quad* __restrict__ tris, int n_faces, const float* __restrict__ aabb_, int G,
                                                               const int32_t* __restrict__ cell_start, int32_t* __restrict__ cursor, int n_list,
                                                               int32_t* __restrict__ cell_list) {
  const float aabb[6] = {aabb_[0], aabb_[1], aabb_[2], aabb_[3], aabb_[4], aabb_[5]};
  for (long f = (long)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += (long)gridDim.x * blockDim.x) {
    const mr::Quad rec[3] = {tris[3 * f], tris[3 * f + 1], tris[3 * f + 2]};
    int i0[3], i1[3];
    if (!mr::face_cells(rec, aabb, G, i0, i1)) continue;
    for (int z = i0[2]; z <= i1[2]; ++z)
      for (int y = i0[1]; y <= i1[1]; ++y)
        for (int x = i0[0]; x <= i1[0]; ++x) {
          const int cell = x + G * (y + G * z);
          const int slot = cell_start[cell] + atomicAdd(&cursor[cell], 1);
          if (slot >= 0 && slot < n_list && slot < cell_start[cell + 1]) cell_list[slot] = (int32_t)f;
        }
  }
}

// One lane per ray, grid-stride.  A lane keeps the ray (o, d: 6), the shear (6), the clip and the best hit (8), the cell, its steps and its
// three wall parameters (9); a face test is three 16-byte loads.  A lane leaves the walk when its ray ends; the wave runs on until its last has.
__global__ void __launch_bounds__(mr::kBlock) k_mesh_raycast(const float* __restrict__ origin, const float* __restrict__ dir, const float* __restrict__ t_range,
                                                              long R, const float* __restrict__ tris, int n_faces, const float* __restrict__ aabb_, int G,
                                                              const int32_t* __restrict__ cell_start, const int32_t* __restrict__ cell_list,
                                                              float* __restrict__ t, int32_t* __restrict__ face, float* __restrict__ u, float* __restrict__ v,
                                                              int32_t* __restrict__ front, int32_t* __restrict__ n_tests) {
  const float aabb[6] = {aabb_[0], aabb_[1], aabb_[2], aabb_[3], aabb_[4], aabb_[5]};
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    const float o[3] = {origin[3 * r], origin[3 * r + 1], origin[3 * r + 2]};
    const float d[3] = {dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    const mr::Hit h = mr::cast_ray(o, d, t_range[2 * r], t_range[2 * r + 1], aabb, G, tris, n_faces, cell_start, cell_list);
    t[r] = h.t, face[r] = h.face, u[r] = h.u, v[r] = h.v, front[r] = h.front, n_tests[r] = h.n_tests;
  }
}

}  // namespace lab4d
using namespace lab4d;

static int check_grid(const char* what, int n_faces, int G) {
  LAB4D_REQUIRE(G >= 1 && G <= mr::kMaxG, "%s: G = %d outside [1, %d]", what, G, mr::kMaxG);
  LAB4D_REQUIRE(n_faces >= 0 && n_faces <= 2147483647 / mr::kTriFloats, "%s: n_faces = %d outside [0, 2^31 / 12]", what, n_faces);
  return LAB4D_OK;
}

extern "C" int lab4d_meshgrid_count(const float* verts, const int32_t* faces, int n_verts, int n_faces, const float* aabb, int G, float* tris,
                                    int32_t* cell_start, int32_t* work, int32_t* total, void* stream) {
  if (int e = check_grid("meshgrid_count", n_faces, G)) return e;
  LAB4D_REQUIRE(n_verts >= 0, "meshgrid_count: n_verts = %d is negative", n_verts);
  if (n_faces == 0) return LAB4D_OK;  // (nothing is read or written: the cast never looks at the lists of an empty mesh)
  LAB4D_REQUIRE(faces && aabb && tris, "meshgrid_count: null pointer (faces, aabb, tris)");
  LAB4D_REQUIRE(n_verts == 0 || verts, "meshgrid_count: null pointer (verts)");
  LAB4D_REQUIRE(cell_start && work && total, "meshgrid_count: null pointer (cell_start, work, total)");
  hipStream_t st = (hipStream_t)stream;
  const int n_cells = G * G * G, nb = (n_cells + mr::kScanBlock - 1) / mr::kScanBlock;
  int32_t* block_sum = work + n_cells;
  if (int e = zero_async(work, (size_t)n_cells * sizeof(int32_t), st)) return e;
  hipLaunchKernelGGL(k_meshgrid_count, dim3(grid_1d(n_faces, mr::kBlock, 2048)), dim3(mr::kBlock), 0, st, verts, faces, n_verts, n_faces, aabb, G, (mr::Quad*)tris,
                     work);
  if (int e = check_launch("meshgrid_count (count)")) return e;
  hipLaunchKernelGGL(k_meshgrid_block_sums, dim3(nb), dim3(256), 0, st, (const int32_t*)work, n_cells, block_sum);
  hipLaunchKernelGGL(k_meshgrid_scan_blocks, dim3(1), dim3(1024), 0, st, block_sum, nb, cell_start + n_cells, total);
  hipLaunchKernelGGL(k_meshgrid_offsets, dim3(nb), dim3(256), 0, st, (const int32_t*)work, n_cells, (const int32_t*)block_sum, cell_start);
  return check_launch("meshgrid_count (scan)");
}

extern "C" int lab4d_meshgrid_pack(const float* verts, const int32_t* faces, int n_verts, int n_faces, float* tris, void* stream) {
  if (int e = check_grid("meshgrid_pack", n_faces, 1)) return e;
  LAB4D_REQUIRE(n_verts >= 0, "meshgrid_pack: n_verts = %d is negative", n_verts);
  if (n_faces == 0) return LAB4D_OK;
  LAB4D_REQUIRE(faces && tris, "meshgrid_pack: null pointer (faces, tris)");
  LAB4D_REQUIRE(n_verts == 0 || verts, "meshgrid_pack: null pointer (verts)");
  hipLaunchKernelGGL(k_meshgrid_pack, dim3(grid_1d(n_faces, mr::kBlock, 2048)), dim3(mr::kBlock), 0, (hipStream_t)stream, verts, faces, n_verts, n_faces,
                     (mr::Quad*)tris);
  return check_launch("meshgrid_pack");
}

extern "C" int lab4d_meshgrid_fill(const float* tris, int n_faces, const float* aabb, int G, const int32_t* cell_start, int32_t* work, int n_list,
                                   int32_t* cell_list, void* stream) {
  if (int e = check_grid("meshgrid_fill", n_faces, G)) return e;
  LAB4D_REQUIRE(n_list >= 0, "meshgrid_fill: n_list = %d is negative", n_list);
  if (n_faces == 0 || n_list == 0) return LAB4D_OK;
  LAB4D_REQUIRE(tris && aabb && cell_start && work && cell_list, "meshgrid_fill: null pointer (tris, aabb, cell_start, work, cell_list)");
  hipStream_t st = (hipStream_t)stream;
  if (int e = zero_async(work, (size_t)G * G * G * sizeof(int32_t), st)) return e;
  hipLaunchKernelGGL(k_meshgrid_fill, dim3(grid_1d(n_faces, mr::kBlock, 2048)), dim3(mr::kBlock), 0, st, (const mr::Quad*)tris, n_faces, aabb, G, cell_start, work,
                     n_list, cell_list);
  return check_launch("meshgrid_fill");
}

extern "C" int lab4d_mesh_raycast(const float* origin, const float* dir, const float* t_range, long R, const float* tris, int n_faces, const float* aabb, int G,
                                  const int32_t* cell_start, const int32_t* cell_list, float* t, int32_t* face, float* u, float* v, int32_t* front,
                                  int32_t* n_tests, void* stream) {
  LAB4D_REQUIRE(R >= 0 && R < (1L << 31), "mesh_raycast: R = %ld outside [0, 2^31)", R);
  if (int e = check_grid("mesh_raycast", n_faces, G)) return e;
  LAB4D_REQUIRE(aabb, "mesh_raycast: null pointer (aabb)");
  LAB4D_REQUIRE(n_faces == 0 || (tris && cell_start), "mesh_raycast: null pointer (tris, cell_start)");
  if (R == 0) return LAB4D_OK;  // (the per-ray arrays are empty: an empty tensor's pointer is NULL)
  LAB4D_REQUIRE(origin && dir && t_range, "mesh_raycast: null pointer (origin, dir, t_range)");
  LAB4D_REQUIRE(t && face && u && v && front && n_tests, "mesh_raycast: null pointer (t, face, u, v, front, n_tests)");
  hipLaunchKernelGGL(k_mesh_raycast, dim3(grid_1d(R, mr::kBlock, 2048)), dim3(mr::kBlock), 0, (hipStream_t)stream, origin, dir, t_range, R, tris, n_faces, aabb, G,
                     cell_start, cell_list, t, face, u, v, front, n_tests);
  return check_launch("mesh_raycast");
}
