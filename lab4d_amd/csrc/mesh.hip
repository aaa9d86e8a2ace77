// Iso-surface extraction of the proxy-geometry refresh -- geom_utils.marching_cubes (lab4d/utils/geom_utils.py:442-503), which copies the
// sdf / visibility volumes to the host for skimage.measure.marching_cubes and trimesh's connected-component split.  Here the volume stays
// where lab4d_amd.proxy.grid_query left it: volume in, welded indexed triangle mesh out.  Contract: include/lab4d_mesh.h; per-cell
// arithmetic: mesh_math.hpp (shared with the CPU twin tests/host_harness/mesh_host.cpp); case table: mc_tables.hpp (generated).
//
// One thread per grid point, consecutive lanes along k (the fastest axis) so that corner loads coalesce; the overlapping corner reads of
// neighbouring lanes are served by L1 / L2 (a 64^3 volume is 1 MB).  Extraction is count -> scan -> write without atomics, the same
// pattern as compact.hip with a wave prefix SUM in place of its ballot (a grid point owns 0..3 vertices, a cell 0..5 triangles):
//   k_mc_classify  cell -> case byte (0 when skipped), per-block triangle counts
//   k_mc_edges     owned edge -> "needs a vertex" flag (crossed and next to a non-empty meshed cell), per-block vertex counts
//   k_mc_scan      one workgroup per count array: exclusive scan, totals -> counts[0..1]
//   k_mc_vertices  vertex positions + the vertex id of every owned edge (int32 lookup volume, -1 where there is none)
//   k_mc_faces     table row -> three lookups in the edge-id volume
// The largest-component filter labels vertices by atomicMin hooking + pointer jumping (ordinary vector atomics), takes the root with
// the most vertices (ties: smallest root = smallest vertex index) and compacts with the same scan.
#include "common.hpp"
#include "mesh_math.hpp"

namespace lab4d {
namespace mc = lab4d_mc;

constexpr int kMcBlock = 256;
constexpr int kCcFlagSlots = 4;  // label passes between two looks at the "changed" flags

struct McLayout {
  long n;       // grid points
  int nb;       // blocks of kMcBlock grid points
  long cases;   // word offsets into the work buffer
  long eflags;
  long vblock;
  long tblock;
  long total;
};

static McLayout mc_layout(int Gx, int Gy, int Gz) {
  McLayout L;
  L.n = (long)Gx * Gy * Gz;
  L.nb = (int)((L.n + kMcBlock - 1) / kMcBlock);
  const long cw = (L.n + 3) / 4;
  L.cases = 3 * L.n;
  L.eflags = L.cases + cw;
  L.vblock = L.eflags + cw;
  L.tblock = L.vblock + L.nb;
  L.total = L.tblock + L.nb;
  return L;
}

static bool mc_shape_ok(int Gx, int Gy, int Gz) {
  return Gx >= 1 && Gy >= 1 && Gz >= 1 && (long)Gx * Gy * Gz < ((1l << 31) / 3);
}

// exclusive prefix sum of v over the 256 threads of a block (thread order); *total = block sum.  s: 4 ints of LDS.
__device__ __forceinline__ int block_scan_excl(int v, int* s, int* total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();  // (s may still be read from a previous call)
  if (lane == 63) s[wid] = incl;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wid; ++w) before += s[w];
  *total = s[0] + s[1] + s[2] + s[3];
  return before + incl - v;
}

__device__ __forceinline__ int block_sum(int v, int* s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return s[0] + s[1] + s[2] + s[3];
}

__global__ void __launch_bounds__(kMcBlock) k_mc_classify(const float* __restrict__ sdf, const unsigned char* __restrict__ mask, int Gx, int Gy, int Gz,
                                                           float level, unsigned char* __restrict__ cases, int* __restrict__ tblock) {
  __shared__ int s[4];
  const long n = (long)Gx * Gy * Gz;
  const long lin = (long)blockIdx.x * kMcBlock + threadIdx.x;
  int ntri = 0;
  if (lin < n) {
    const int k = (int)(lin % Gz), j = (int)((lin / Gz) % Gy), i = (int)(lin / ((long)Gz * Gy));
    int cs = 0;
    if (i + 1 < Gx && j + 1 < Gy && k + 1 < Gz) {
      float v[8];
      unsigned char m[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const long o = lin + mc::corner_offset(c, Gy, Gz);
        v[c] = sdf[o];
        m[c] = mask ? mask[o] : (unsigned char)1;
      }
      if (mc::cell_meshed(v, m)) cs = mc::cell_case(v, level);
    }
    cases[lin] = (unsigned char)cs;
    ntri = mc::kTriCount[cs];
  }
  const int tot = block_sum(ntri, s);
  if (threadIdx.x == 0) tblock[blockIdx.x] = tot;
}

// bit a of the result: the +axis-a edge owned by grid point (i, j, k) carries a vertex
__device__ __forceinline__ int owned_edge_flags(const float* __restrict__ sdf, const unsigned char* __restrict__ cases, int Gx, int Gy, int Gz, float level,
                                                long lin, int i, int j, int k) {
  const int G[3] = {Gx, Gy, Gz}, p[3] = {i, j, k};
  const long stride[3] = {(long)Gy * Gz, (long)Gz, 1};
  const float v0 = sdf[lin];
  int f = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (p[a] + 1 >= G[a]) continue;
    if (!mc::edge_crossed(v0, sdf[lin + stride[a]], level)) continue;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    bool any = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // the cells around the edge: p - {0,1} e_b - {0,1} e_c (cases[] is 0 at non-cells)
      const int db = q & 1, dc = q >> 1;
      if (p[b] - db < 0 || p[c] - dc < 0) continue;
      any = any || cases[lin - db * stride[b] - dc * stride[c]] != 0;
    }
    if (any) f |= 1 << a;
  }
  return f;
}

__global__ void __launch_bounds__(kMcBlock) k_mc_edges(const float* __restrict__ sdf, const unsigned char* __restrict__ cases, int Gx, int Gy, int Gz, float level,
                                                        unsigned char* __restrict__ eflags, int* __restrict__ vblock) {
  __shared__ int s[4];
  const long n = (long)Gx * Gy * Gz;
  const long lin = (long)blockIdx.x * kMcBlock + threadIdx.x;
  int f = 0;
  if (lin < n) {
    const int k = (int)(lin % Gz), j = (int)((lin / Gz) % Gy), i = (int)(lin / ((long)Gz * Gy));
    f = owned_edge_flags(sdf, cases, Gx, Gy, Gz, level, lin, i, j, k);
    eflags[lin] = (unsigned char)f;
  }
  const int tot = block_sum(__popc(f), s);
  if (threadIdx.x == 0) vblock[blockIdx.x] = tot;
}

// exclusive scan of two count arrays, one workgroup each (blockIdx.x = which); totals -> totals[which]
__global__ void __launch_bounds__(1024) k_mc_scan(int* __restrict__ a0, int* __restrict__ a1, int n, int* __restrict__ totals) {
  __shared__ int part[1024];
  int* a = blockIdx.x ? a1 : a0;
  const int per = (n + 1023) / 1024;
  const long b0 = (long)threadIdx.x * per;
  int sum = 0;
  for (int i = 0; i < per; ++i)
    if (b0 + i < n) sum += a[b0 + i];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
    const int v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int run = threadIdx.x ? part[threadIdx.x - 1] : 0;
  for (int i = 0; i < per; ++i)
    if (b0 + i < n) {
      const int c = a[b0 + i];
      a[b0 + i] = run;
      run += c;
    }
  if (threadIdx.x == 1023) totals[blockIdx.x] = part[1023];
}

__global__ void __launch_bounds__(kMcBlock) k_mc_vertices(const float* __restrict__ sdf, const unsigned char* __restrict__ eflags, int Gx, int Gy, int Gz,
                                                           float level, const float* __restrict__ xform, const int* __restrict__ vblock, int n_verts,
                                                           int* __restrict__ edge_id, float* __restrict__ verts) {
  __shared__ int s[4];
  const long n = (long)Gx * Gy * Gz;
  const long lin = (long)blockIdx.x * kMcBlock + threadIdx.x;
  const int f = lin < n ? eflags[lin] : 0;
  int tot;
  int id = vblock[blockIdx.x] + block_scan_excl(__popc(f), s, &tot);
  if (lin >= n) return;
  const int p[3] = {(int)(lin / ((long)Gz * Gy)), (int)((lin / Gz) % Gy), (int)(lin % Gz)};
  const long stride[3] = {(long)Gy * Gz, (long)Gz, 1};
  const float v0 = f ? sdf[lin] : 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const bool on = (f >> a) & 1;
    edge_id[lin * 3 + a] = on ? id : -1;
    if (on && id < n_verts) {
      float q[3] = {(float)p[0], (float)p[1], (float)p[2]};
      q[a] = mc::edge_vertex(p[a], v0, sdf[lin + stride[a]], level);
#pragma unroll
      for (int d = 0; d < 3; ++d) verts[(long)id * 3 + d] = xform ? mc::to_world(q[d], xform[d], xform[3 + d]) : q[d];
    }
    id += on ? 1 : 0;
  }
}

__global__ void __launch_bounds__(kMcBlock) k_mc_faces(const unsigned char* __restrict__ cases, int Gx, int Gy, int Gz, const int* __restrict__ tblock,
                                                        const int* __restrict__ edge_id, int n_faces, int* __restrict__ faces) {
  // the table is indexed by a per-lane case: LDS, not the scalar / constant path
  __shared__ unsigned char tri_edges[256 * 3 * mc::kMaxTris];
  __shared__ unsigned char tri_count[256];
  __shared__ long edge_off[12];
  __shared__ int s[4];
  for (int e = threadIdx.x; e < 256 * 3 * mc::kMaxTris; e += kMcBlock) tri_edges[e] = mc::kTriEdges[e / (3 * mc::kMaxTris)][e % (3 * mc::kMaxTris)];
  tri_count[threadIdx.x] = mc::kTriCount[threadIdx.x];
  if (threadIdx.x < 12) edge_off[threadIdx.x] = mc::corner_offset(mc::kEdgeCorner[threadIdx.x], Gy, Gz) * 3 + mc::kEdgeAxis[threadIdx.x];
  __syncthreads();
  const long n = (long)Gx * Gy * Gz;
  const long lin = (long)blockIdx.x * kMcBlock + threadIdx.x;
  const int cs = lin < n ? cases[lin] : 0;
  const int nt = tri_count[cs];
  int tot;
  const int base = tblock[blockIdx.x] + block_scan_excl(nt, s, &tot);
  for (int t = 0; t < nt; ++t) {
    if (base + t >= n_faces) break;
#pragma unroll
    for (int m = 0; m < 3; ++m) faces[(long)(base + t) * 3 + m] = edge_id[lin * 3 + edge_off[tri_edges[cs * 3 * mc::kMaxTris + 3 * t + m]]];
  }
}

// ---------------------------------------------------------------------------------------------------
// largest connected component
// ---------------------------------------------------------------------------------------------------
struct CcLayout {
  int nb;  // blocks of kMcBlock over max(n_verts, n_faces)
  long parent, size, remap, vblock, fblock, flags, winner, total;
};

static CcLayout cc_layout(int n_verts, int n_faces) {
  CcLayout L;
  const long m = n_verts > n_faces ? n_verts : n_faces;
  L.nb = (int)((m + kMcBlock - 1) / kMcBlock);
  L.parent = 0;
  L.size = L.parent + n_verts;
  L.remap = L.size + n_verts;
  L.vblock = L.remap + n_verts;
  L.fblock = L.vblock + L.nb;
  L.flags = L.fblock + L.nb;
  L.winner = (L.flags + kCcFlagSlots + 1) & ~1l;  // 8-byte aligned (the work buffer is)
  L.total = L.winner + 2;
  return L;
}

__device__ __forceinline__ int cc_root(const int* parent, int v) {
  // parent[x] <= x always (hooks go to the smaller label), so the walk ends; a concurrent atomicMin only shortens it
  int p = __atomic_load_n(parent + v, __ATOMIC_RELAXED);
  while (p != v) {
    v = p;
    p = __atomic_load_n(parent + v, __ATOMIC_RELAXED);
  }
  return v;
}

__global__ void __launch_bounds__(256) k_cc_init(int* __restrict__ parent, int* __restrict__ size, int n_verts, int* __restrict__ flags,
                                                  unsigned long long* __restrict__ winner) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < n_verts) {
    parent[v] = v;
    size[v] = 0;
  }
  if (v < kCcFlagSlots) flags[v] = 0;
  if (v == 0) *winner = 0ull;
}

__global__ void __launch_bounds__(256) k_cc_clear_flags(int* __restrict__ flags) {
  if (threadIdx.x < kCcFlagSlots) flags[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(256) k_cc_hook(const int* __restrict__ faces, int n_faces, int n_verts, int* parent, int* __restrict__ flag) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= n_faces) return;
  int r[3];
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int v = faces[(long)f * 3 + m];
    if (v < 0 || v >= n_verts) return;  // (not a face of this mesh: never produced by lab4d_mesh_emit)
    r[m] = cc_root(parent, v);
  }
  const int lo = min(r[0], min(r[1], r[2]));
  bool changed = false;
#pragma unroll
  for (int m = 0; m < 3; ++m)
    if (r[m] != lo) {
      atomicMin(parent + r[m], lo);
      changed = true;
    }
  if (changed) *flag = 1;
}

__global__ void __launch_bounds__(256) k_cc_jump(int* parent, int n_verts) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < n_verts) {
    const int r = cc_root(parent, v);
    if (r != v) __atomic_store_n(parent + v, r, __ATOMIC_RELAXED);
  }
}

__global__ void __launch_bounds__(256) k_cc_hist(const int* __restrict__ parent, int n_verts, int* __restrict__ size) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < n_verts) atomicAdd(size + parent[v], 1);
}

// key = (size << 32) | (INT_MAX - root): the maximum is the largest component, ties to the smaller root
__global__ void __launch_bounds__(256) k_cc_winner(const int* __restrict__ parent, const int* __restrict__ size, int n_verts,
                                                    unsigned long long* __restrict__ winner) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < n_verts && parent[v] == v) atomicMax(winner, ((unsigned long long)(unsigned)size[v] << 32) | (unsigned)(0x7fffffff - v));
}

__device__ __forceinline__ int cc_winner_root(const unsigned long long* winner) { return 0x7fffffff - (int)(*winner & 0xffffffffull); }

// a face survives iff its vertices belong to the winner (one test suffices for a face of this mesh; indices are range-checked like in k_cc_hook)
__device__ __forceinline__ bool cc_face_kept(const int* __restrict__ parent, const int* __restrict__ faces, int f, int n_verts, int w) {
  const int a = faces[(long)f * 3], b = faces[(long)f * 3 + 1], c = faces[(long)f * 3 + 2];
  if (a < 0 || b < 0 || c < 0 || a >= n_verts || b >= n_verts || c >= n_verts) return false;
  return parent[a] == w;
}

__global__ void __launch_bounds__(kMcBlock) k_cc_count(const int* __restrict__ parent, const int* __restrict__ faces, int n_verts, int n_faces,
                                                        const unsigned long long* __restrict__ winner, int* __restrict__ vblock, int* __restrict__ fblock) {
  __shared__ int s[4];
  const int w = cc_winner_root(winner);
  const int e = blockIdx.x * kMcBlock + threadIdx.x;
  const int kv = (e < n_verts && parent[e] == w) ? 1 : 0;
  const int kf = (e < n_faces && cc_face_kept(parent, faces, e, n_verts, w)) ? 1 : 0;
  const int tv = block_sum(kv, s);
  const int tf = block_sum(kf, s);
  if (threadIdx.x == 0) {
    vblock[blockIdx.x] = tv;
    fblock[blockIdx.x] = tf;
  }
}

__global__ void __launch_bounds__(kMcBlock) k_cc_write_verts(const int* __restrict__ parent, const float* __restrict__ verts, int n_verts,
                                                              const unsigned long long* __restrict__ winner, const int* __restrict__ vblock,
                                                              int* __restrict__ remap, float* __restrict__ out_verts) {
  __shared__ int s[4];
  const int w = cc_winner_root(winner);
  const int v = blockIdx.x * kMcBlock + threadIdx.x;
  const int keep = (v < n_verts && parent[v] == w) ? 1 : 0;
  int tot;
  const int id = vblock[blockIdx.x] + block_scan_excl(keep, s, &tot);
  if (v >= n_verts) return;
  remap[v] = keep ? id : -1;
  if (keep) {
#pragma unroll
    for (int d = 0; d < 3; ++d) out_verts[(long)id * 3 + d] = verts[(long)v * 3 + d];
  }
}

__global__ void __launch_bounds__(kMcBlock) k_cc_write_faces(const int* __restrict__ parent, const int* __restrict__ faces, int n_verts, int n_faces,
                                                              const unsigned long long* __restrict__ winner, const int* __restrict__ fblock,
                                                              const int* __restrict__ remap, int* __restrict__ out_faces) {
  __shared__ int s[4];
  const int w = cc_winner_root(winner);
  const int f = blockIdx.x * kMcBlock + threadIdx.x;
  const int keep = (f < n_faces && cc_face_kept(parent, faces, f, n_verts, w)) ? 1 : 0;
  int tot;
  const int id = fblock[blockIdx.x] + block_scan_excl(keep, s, &tot);
  if (keep) {
#pragma unroll
    for (int m = 0; m < 3; ++m) out_faces[(long)id * 3 + m] = remap[faces[(long)f * 3 + m]];
  }
}

}  // namespace lab4d
using namespace lab4d;

extern "C" int64_t lab4d_mesh_work_ints(int Gx, int Gy, int Gz) {
  if (!mc_shape_ok(Gx, Gy, Gz)) return -1;
  return mc_layout(Gx, Gy, Gz).total;
}

extern "C" int lab4d_mesh_count(const float* sdf, const unsigned char* mask, int Gx, int Gy, int Gz, float level, int32_t* work, int32_t* counts,
                                void* stream) {
  LAB4D_REQUIRE(sdf && work && counts, "mesh_count: null pointer");
  LAB4D_REQUIRE(Gx >= 1 && Gy >= 1 && Gz >= 1, "mesh_count: grid dimensions must be >= 1 (got %d x %d x %d)", Gx, Gy, Gz);
  LAB4D_REQUIRE(mc_shape_ok(Gx, Gy, Gz), "mesh_count: grid too large (%d x %d x %d points; Gx * Gy * Gz must stay below 2^31 / 3)", Gx, Gy, Gz);
  LAB4D_REQUIRE(level == level, "mesh_count: level is NaN");
  const McLayout L = mc_layout(Gx, Gy, Gz);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* cases = (unsigned char*)(work + L.cases);
  unsigned char* eflags = (unsigned char*)(work + L.eflags);
  hipLaunchKernelGGL(k_mc_classify, dim3(L.nb), dim3(kMcBlock), 0, st, sdf, mask, Gx, Gy, Gz, level, cases, work + L.tblock);
  hipLaunchKernelGGL(k_mc_edges, dim3(L.nb), dim3(kMcBlock), 0, st, sdf, (const unsigned char*)cases, Gx, Gy, Gz, level, eflags, work + L.vblock);
  hipLaunchKernelGGL(k_mc_scan, dim3(2), dim3(1024), 0, st, work + L.vblock, work + L.tblock, L.nb, counts);
  return check_launch("mesh_count");
}

extern "C" int lab4d_mesh_emit(const float* sdf, int Gx, int Gy, int Gz, float level, const float* xform, int32_t* work, int n_verts, int n_faces,
                               float* verts, int32_t* faces, void* stream) {
  LAB4D_REQUIRE(sdf && work, "mesh_emit: null pointer");
  LAB4D_REQUIRE(Gx >= 1 && Gy >= 1 && Gz >= 1, "mesh_emit: grid dimensions must be >= 1 (got %d x %d x %d)", Gx, Gy, Gz);
  LAB4D_REQUIRE(mc_shape_ok(Gx, Gy, Gz), "mesh_emit: grid too large (%d x %d x %d points; Gx * Gy * Gz must stay below 2^31 / 3)", Gx, Gy, Gz);
  LAB4D_REQUIRE(n_verts >= 0 && n_faces >= 0, "mesh_emit: negative n_verts / n_faces");
  LAB4D_REQUIRE((n_verts == 0 || verts) && (n_faces == 0 || faces), "mesh_emit: null output");
  const McLayout L = mc_layout(Gx, Gy, Gz);
  LAB4D_REQUIRE(n_verts <= 3 * L.n && n_faces <= (long)lab4d_mc::kMaxTris * L.n, "mesh_emit: n_verts / n_faces exceed what this grid can produce");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mc_vertices, dim3(L.nb), dim3(kMcBlock), 0, st, sdf, (const unsigned char*)(work + L.eflags), Gx, Gy, Gz, level, xform,
                     (const int*)(work + L.vblock), n_verts, work, verts);
  if (n_faces > 0)
    hipLaunchKernelGGL(k_mc_faces, dim3(L.nb), dim3(kMcBlock), 0, st, (const unsigned char*)(work + L.cases), Gx, Gy, Gz, (const int*)(work + L.tblock),
                       (const int*)work, n_faces, faces);
  return check_launch("mesh_emit");
}

extern "C" int64_t lab4d_mesh_component_work_ints(int n_verts, int n_faces) {
  if (n_verts < 0 || n_faces < 0) return -1;
  return cc_layout(n_verts, n_faces).total;
}

extern "C" int lab4d_mesh_largest_component(const float* verts, const int32_t* faces, int n_verts, int n_faces, int32_t* work, float* out_verts,
                                            int32_t* out_faces, int32_t* out_counts, int* stats, void* stream) {
  LAB4D_REQUIRE(n_verts >= 0 && n_faces >= 0, "mesh_largest_component: negative n_verts / n_faces");
  LAB4D_REQUIRE(out_counts && work, "mesh_largest_component: null pointer");
  LAB4D_REQUIRE((n_verts == 0 || (verts && out_verts)) && (n_faces == 0 || (faces && out_faces)), "mesh_largest_component: null pointer");
  LAB4D_REQUIRE(((uintptr_t)work & 7) == 0, "mesh_largest_component: work must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (stats) stats[0] = stats[1] = 0;
  if (n_verts == 0) return zero_async(out_counts, 2 * sizeof(int32_t), st);
  const CcLayout L = cc_layout(n_verts, n_faces);
  int* parent = work + L.parent;
  int* size = work + L.size;
  int* flags = work + L.flags;
  unsigned long long* winner = (unsigned long long*)(work + L.winner);
  const int gv = div_up(n_verts, 256), gf = div_up(n_faces, 256);
  hipLaunchKernelGGL(k_cc_init, dim3(gv), dim3(256), 0, st, parent, size, n_verts, flags, winner);
  int passes = 0, reads = 0;
  while (n_faces > 0) {
    // kCcFlagSlots passes, then ONE look at their flags: once a pass changes nothing, no later pass does
    for (int p = 0; p < kCcFlagSlots; ++p) {
      hipLaunchKernelGGL(k_cc_hook, dim3(gf), dim3(256), 0, st, faces, n_faces, n_verts, parent, flags + p);
      hipLaunchKernelGGL(k_cc_jump, dim3(gv), dim3(256), 0, st, parent, n_verts);
    }
    passes += kCcFlagSlots;
    int h[kCcFlagSlots];
    hipError_t e = hipMemcpyAsync(h, flags, sizeof(h), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      set_error("mesh_largest_component: %s", hipGetErrorString(e));
      return LAB4D_ELAUNCH;
    }
    ++reads;
    if (h[kCcFlagSlots - 1] == 0) break;
    hipLaunchKernelGGL(k_cc_clear_flags, dim3(1), dim3(256), 0, st, flags);
  }
  hipLaunchKernelGGL(k_cc_hist, dim3(gv), dim3(256), 0, st, (const int*)parent, n_verts, size);
  hipLaunchKernelGGL(k_cc_winner, dim3(gv), dim3(256), 0, st, (const int*)parent, (const int*)size, n_verts, winner);
  hipLaunchKernelGGL(k_cc_count, dim3(L.nb), dim3(kMcBlock), 0, st, (const int*)parent, faces, n_verts, n_faces, (const unsigned long long*)winner,
                     work + L.vblock, work + L.fblock);
  hipLaunchKernelGGL(k_mc_scan, dim3(2), dim3(1024), 0, st, work + L.vblock, work + L.fblock, L.nb, out_counts);
  hipLaunchKernelGGL(k_cc_write_verts, dim3(L.nb), dim3(kMcBlock), 0, st, (const int*)parent, verts, n_verts, (const unsigned long long*)winner,
                     (const int*)(work + L.vblock), work + L.remap, out_verts);
  if (n_faces > 0)
    hipLaunchKernelGGL(k_cc_write_faces, dim3(L.nb), dim3(kMcBlock), 0, st, (const int*)parent, faces, n_verts, n_faces, (const unsigned long long*)winner,
                       (const int*)(work + L.fblock), (const int*)(work + L.remap), out_faces);
  if (stats) {
    stats[0] = passes;
    stats[1] = reads;
  }
  return check_launch("mesh_largest_component");
}
