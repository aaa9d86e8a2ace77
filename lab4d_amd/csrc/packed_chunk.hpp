// The weights of 64 consecutive rows of a packed ray (device only): the one chunked scan of tau behind lab4d_packed_composite_forward /
// _backward (packed.hip) and lab4d_packed_distortion_forward / _backward (distort.hip), so that every consumer of a packed list sees the
// same w_i on the same rows.  One 64-lane wave per ray, lanes over the ray's consecutive rows: composite.hip's wave scan with the carry
// between the chunks.
#pragma once
#include "common.hpp"
#include "packed_math.hpp"

namespace lab4d {
namespace pk = lab4d_packed;

struct ChunkWeights {
  float w, T;
};
// carry: sum of tau over the chunks before this one on entry, this one included on exit
__device__ __forceinline__ ChunkWeights chunk_weights(const float* __restrict__ density, const float* __restrict__ deltas, long row, bool live, int lane,
                                                      float& carry) {
  const float tau = live ? density[row] * deltas[row] : 0.f;
  const float incl = wave_scan_incl(tau, lane) + carry;
  float excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = carry;
  carry = __shfl(incl, 63, 64);
  return {live ? pk::weight_of(tau, excl) : 0.f, pk::transmit_of(incl)};
}

}  // namespace lab4d
