// Camera-visibility culling of the occupancy grids: mark the cells that at least min_views of M camera frusta see, and apply the mark to a
// grid's bits, ema and count.  Contract: include/lab4d_occvis.h; every rule and all of the arithmetic: occvis_math.hpp, shared with the CPU
// twin tests/host_harness/occvis/occvis_host.cpp, to which these kernels are held word for word.  Nothing here reads back or allocates: both
// entry points can be captured in a hipGraph.
#include "common.hpp"
#include "occvis_math.hpp"

namespace lab4d {
namespace occ = lab4d_occ;
namespace occv = lab4d_occvis;

// One lane per cell, blocks of 4 waves, blockIdx.y = the level; wave w of a level owns cells [64 w, 64 w + 64) = words 2 w and 2 w + 1, as
// k_occgrid_update.  The planes are the same for every cell: a tile of kTile views (6 KB) is staged through LDS with 16-byte loads, lane
// t < tile checks view t's coefficients once, and every lane then reads the same LDS address (a broadcast, no bank conflict).  A wave
// leaves the loop over the views once none of its cells is still short of min_views (one ballot per view); it keeps taking part in the
// staging of the block's later tiles, and the block leaves when all four waves have (__syncthreads_and, which is also the barrier in front
// of the next tile's stores).  With min_views = 1 a cell in front of the cameras costs a handful of views, a cell nobody sees all M.
__global__ void __launch_bounds__(256) k_occvis_mark(const float4* __restrict__ planes, int M, const float* __restrict__ aabbs, int G, int min_views,
                                                      uint32_t* __restrict__ vis_bits, int32_t* __restrict__ n_visible, long n, long n_words) {
  __shared__ float4 s_planes[occv::kTile * 6];
  __shared__ int s_valid[occv::kTile];
  const int level = blockIdx.y;
  const float* aabb = aabbs + 6 * level;
  const float box[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = idx < n;
  float c[3], h[3], q[3];
  occv::cell_box(live ? idx : 0, box, G, c, h, q);
  int seen = 0;
  bool done = __ballot(live) == 0;  // (wave-uniform from here on)
  for (int m0 = 0; m0 < M; m0 += occv::kTile) {
    const int nv = M - m0 < occv::kTile ? M - m0 : occv::kTile;
    for (int e = threadIdx.x; e < nv * 6; e += 256) s_planes[e] = planes[(long)m0 * 6 + e];
    __syncthreads();
    if ((int)threadIdx.x < nv) s_valid[threadIdx.x] = occv::view_finite((const float*)&s_planes[threadIdx.x * 6]) ? 1 : 0;
    __syncthreads();
    if (!done) {
      for (int v = 0; v < nv; ++v) {
        if (!s_valid[v]) continue;
        if (live && seen < min_views && occv::view_sees((const float*)&s_planes[v * 6], c, h, q)) ++seen;
        if (__ballot(live && seen < min_views) == 0) {
          done = true;
          break;
        }
      }
    }
    if (__syncthreads_and(done ? 1 : 0)) break;
  }
  const unsigned long long vote = __ballot(live && seen >= min_views);  // lanes behind the last cell vote 0: the padding bits are zero
  if ((threadIdx.x & 63) == 0) {
    const long w = idx >> 5;  // idx is this wave's first cell, a multiple of 64
    uint32_t* words = vis_bits + (long)level * n_words;
    if (w < n_words) words[w] = (uint32_t)vote;
    if (w + 1 < n_words) words[w + 1] = (uint32_t)(vote >> 32);
    if (vote) atomicAdd(n_visible + level, __popcll(vote));
  }
}

// One lane per cell, the layout of k_occvis_mark: bits &= vis, ema = 0 where invisible, n_occupied = the popcount of the new words.
__global__ void __launch_bounds__(256) k_occvis_apply(const uint32_t* __restrict__ vis_bits, float* __restrict__ ema, uint32_t* __restrict__ bits,
                                                       int32_t* __restrict__ n_occupied, long n, long n_words) {
  const int level = blockIdx.y;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  uint32_t* words = bits + (long)level * n_words;
  bool on = false;
  if (idx < n) {
    float e = ema[(long)level * n + idx];
    const bool vis = occ::bit_of(vis_bits + (long)level * n_words, idx);
    on = occv::apply_cell(occ::bit_of(words, idx), vis, &e);
    if (!vis) ema[(long)level * n + idx] = e;
  }
  const unsigned long long vote = __ballot(on);  // (every lane of the wave has read its word before lane 0 stores it: the ballot waits for all)
  if ((threadIdx.x & 63) == 0) {
    const long w = idx >> 5;
    if (w < n_words) words[w] = (uint32_t)vote;
    if (w + 1 < n_words) words[w + 1] = (uint32_t)(vote >> 32);
    if (vote) atomicAdd(n_occupied + level, __popcll(vote));
  }
}

}  // namespace lab4d
using namespace lab4d;

static int check_levels(const char* what, int K, int G) {
  LAB4D_REQUIRE(K >= lab4d_occvis::kMinK && K <= lab4d_occvis::kMaxK, "%s: K = %d outside [%d, %d]", what, K, lab4d_occvis::kMinK, lab4d_occvis::kMaxK);
  LAB4D_REQUIRE(G >= lab4d_occ::kMinG && G <= lab4d_occ::kMaxG, "%s: G = %d outside [%d, %d]", what, G, lab4d_occ::kMinG, lab4d_occ::kMaxG);
  return LAB4D_OK;
}

extern "C" int lab4d_occvis_mark(const float* planes, int M, const float* aabbs, int K, int G, int min_views, uint32_t* vis_bits, int32_t* n_visible,
                                 void* stream) {
  LAB4D_REQUIRE(M >= 1 && M <= lab4d_occvis::kMaxM, "occvis_mark: M = %d outside [1, %d]", M, lab4d_occvis::kMaxM);
  if (int e = check_levels("occvis_mark", K, G)) return e;
  LAB4D_REQUIRE(min_views >= 1 && min_views <= M, "occvis_mark: min_views = %d outside [1, M = %d]", min_views, M);
  LAB4D_REQUIRE(planes && aabbs && vis_bits && n_visible, "occvis_mark: null pointer");
  LAB4D_REQUIRE(((uintptr_t)planes & 15) == 0, "occvis_mark: planes must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (int e = zero_async(n_visible, K * sizeof(int32_t), st)) return e;
  const long n = lab4d_occ::n_cells(G);
  hipLaunchKernelGGL(k_occvis_mark, dim3((unsigned)((n + 255) / 256), (unsigned)K), dim3(256), 0, st, (const float4*)planes, M, aabbs, G, min_views, vis_bits,
                     n_visible, n, lab4d_occ::n_words(G));
  return check_launch("occvis_mark");
}

extern "C" int lab4d_occvis_apply(const uint32_t* vis_bits, float* ema, uint32_t* bits, int32_t* n_occupied, int K, int G, void* stream) {
  if (int e = check_levels("occvis_apply", K, G)) return e;
  LAB4D_REQUIRE(vis_bits && ema && bits && n_occupied, "occvis_apply: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (int e = zero_async(n_occupied, K * sizeof(int32_t), st)) return e;
  const long n = lab4d_occ::n_cells(G);
  hipLaunchKernelGGL(k_occvis_apply, dim3((unsigned)((n + 255) / 256), (unsigned)K), dim3(256), 0, st, vis_bits, ema, bits, n_occupied, n, lab4d_occ::n_words(G));
  return check_launch("occvis_apply");
}
