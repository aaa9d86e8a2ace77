// Occupancy bit grid of the hash field: refresh from a density volume, per-sample mask, per-ray span.  Contract: include/lab4d_occgrid.h;
// every rule and all of the arithmetic: occgrid_math.hpp, shared with the CPU twin tests/host_harness/occgrid_host.cpp, to which these
// kernels are held bit for bit.  Nothing here reads back or allocates: all three entry points can be captured in a hipGraph.
#include "common.hpp"
#include "occgrid_math.hpp"

namespace lab4d {
namespace occ = lab4d_occ;

// One lane per cell, blocks of 4 waves; wave w of the grid owns cells [64 w, 64 w + 64) = words 2 w and 2 w + 1.  Lanes behind the last
// cell vote 0, so the padding bits of the last word are zero whatever the lane count; a word is stored iff it exists (the GRID's tail:
// n_words is odd when G^3 mod 64 is in 1..32).
__global__ void __launch_bounds__(256) k_occgrid_update(const float* __restrict__ density, float* __restrict__ ema, uint32_t* __restrict__ bits,
                                                         int32_t* __restrict__ n_occupied, long n, long n_words, float decay, float thresh) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  bool on = false;
  if (idx < n) {
    const float e = occ::ema_next(ema[idx], density[idx], decay);
    ema[idx] = e;
    on = occ::occupied(e, thresh);
  }
  const unsigned long long vote = __ballot(on);  // the same value in every lane
  if ((threadIdx.x & 63) == 0) {
    const long w = idx >> 5;  // idx is this wave's first cell, a multiple of 64
    if (w < n_words) bits[w] = (uint32_t)vote;
    if (w + 1 < n_words) bits[w + 1] = (uint32_t)(vote >> 32);
    if (vote) atomicAdd(n_occupied, __popcll(vote));
  }
}

__global__ void __launch_bounds__(256) k_occgrid_mask(const float* __restrict__ xyz, const float* __restrict__ aabb, const uint32_t* __restrict__ bits,
                                                       int G, long S, uint8_t* __restrict__ mask) {
  const float box[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
  for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (long)gridDim.x * blockDim.x) {
    const float p[3] = {xyz[3 * s], xyz[3 * s + 1], xyz[3 * s + 2]};
    mask[s] = occ::sample_mask(p, box, bits, G) ? 1 : 0;
  }
}

// One lane per ray.  The bit grid (256 KB at G = 128) is read through the caches: neighbouring rays walk neighbouring cells, and a
// workgroup's LDS could not hold it anyway.  The walk is bounded by 3 * G cells inside occ::ray_span.
__global__ void __launch_bounds__(256) k_occgrid_ray_span(const float* __restrict__ origin, const float* __restrict__ dir, const float* __restrict__ t_range,
                                                           const float* __restrict__ aabb, const uint32_t* __restrict__ bits, int G, long R,
                                                           float* __restrict__ t_span, uint8_t* __restrict__ hit) {
  const float box[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    const float o[3] = {origin[3 * r], origin[3 * r + 1], origin[3 * r + 2]};
    const float d[3] = {dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    float span[2];
    const bool h = occ::ray_span(o, d, t_range[2 * r], t_range[2 * r + 1], box, bits, G, span, nullptr);
    t_span[2 * r] = span[0];
    t_span[2 * r + 1] = span[1];
    hit[r] = h ? 1 : 0;
  }
}

}  // namespace lab4d
using namespace lab4d;

#define LAB4D_OCC_REQUIRE_G(what) \
  LAB4D_REQUIRE(G >= lab4d_occ::kMinG && G <= lab4d_occ::kMaxG, what ": G = %d outside [%d, %d]", G, lab4d_occ::kMinG, lab4d_occ::kMaxG)

extern "C" int lab4d_occgrid_update(const float* density, float* ema, uint32_t* bits, int32_t* n_occupied, int G, float decay, float thresh,
                                    void* stream) {
  LAB4D_REQUIRE(density && ema && bits && n_occupied, "occgrid_update: null pointer");
  LAB4D_OCC_REQUIRE_G("occgrid_update");
  LAB4D_REQUIRE(decay >= 0.f && decay <= 1.f, "occgrid_update: decay %g outside [0, 1]", (double)decay);
  LAB4D_REQUIRE(thresh >= 0.f && thresh < 3.0e38f, "occgrid_update: thresh %g must be finite and >= 0", (double)thresh);
  hipStream_t st = (hipStream_t)stream;
  if (int e = zero_async(n_occupied, sizeof(int32_t), st)) return e;
  const long n = lab4d_occ::n_cells(G);
  hipLaunchKernelGGL(k_occgrid_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, density, ema, bits, n_occupied, n, lab4d_occ::n_words(G), decay,
                     thresh);
  return check_launch("occgrid_update");
}

extern "C" int lab4d_occgrid_mask(const float* xyz, const float* aabb, const uint32_t* bits, int G, long S, uint8_t* mask, void* stream) {
  LAB4D_REQUIRE(S >= 0, "occgrid_mask: S < 0");
  LAB4D_OCC_REQUIRE_G("occgrid_mask");
  if (S == 0) return LAB4D_OK;
  LAB4D_REQUIRE(xyz && aabb && bits && mask, "occgrid_mask: null pointer");
  hipLaunchKernelGGL(k_occgrid_mask, dim3(grid_1d(S, 256, 8192)), dim3(256), 0, (hipStream_t)stream, xyz, aabb, bits, G, S, mask);
  return check_launch("occgrid_mask");
}

extern "C" int lab4d_occgrid_ray_span(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G,
                                      long R, float* t_span, uint8_t* hit, void* stream) {
  LAB4D_REQUIRE(R >= 0, "occgrid_ray_span: R < 0");
  LAB4D_OCC_REQUIRE_G("occgrid_ray_span");
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(origin && dir && t_range && aabb && bits && t_span && hit, "occgrid_ray_span: null pointer");
  hipLaunchKernelGGL(k_occgrid_ray_span, dim3(grid_1d(R, 256, 8192)), dim3(256), 0, (hipStream_t)stream, origin, dir, t_range, aabb, bits, G, R, t_span, hit);
  return check_launch("occgrid_ray_span");
}
