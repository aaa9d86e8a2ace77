// Packed ray marching and ragged compositing of the hash field.  Contract: include/lab4d_packed.h; every rule and the march's arithmetic:
// packed_math.hpp (over occgrid_math.hpp), shared with the CPU twin tests/host_harness/packed_host.cpp, to which the two march kernels are
// held word for word.  Nothing here reads back or allocates: every entry point can be captured in a hipGraph.
#include "common.hpp"
#include "packed_chunk.hpp"
#include "packed_math.hpp"

namespace lab4d {
namespace occ = lab4d_occ;
namespace pk = lab4d_packed;

// ---- march ----------------------------------------------------------------------------------------------------------------------------
// One lane per ray, as k_occgrid_ray_span: the walk over the cells, then the ray's own lattice between the first and the last occupied cell.
__global__ void __launch_bounds__(256) k_packed_march_count(const float* __restrict__ origin, const float* __restrict__ dir, const float* __restrict__ t_range,
                                                             const float* __restrict__ aabb, const uint32_t* __restrict__ bits, int G, long R, float dt,
                                                             int k_max, int32_t* __restrict__ ray_count) {
  const float box[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    const float o[3] = {origin[3 * r], origin[3 * r + 1], origin[3 * r + 2]};
    const float d[3] = {dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    ray_count[r] = pk::march_ray(o, d, t_range[2 * r], t_range[2 * r + 1], box, bits, G, dt, k_max, [](int, float, const float*) {});
  }
}

// The same march again; sample i of ray r goes to row ray_start[r] + i when that row lies below the capacity.  The last ray knows the total.
__global__ void __launch_bounds__(256) k_packed_march_write(const float* __restrict__ origin, const float* __restrict__ dir, const float* __restrict__ t_range,
                                                             const float* __restrict__ aabb, const uint32_t* __restrict__ bits, int G, long R, float dt,
                                                             int k_max, const int32_t* __restrict__ ray_start, long cap, float* __restrict__ t_out,
                                                             float* __restrict__ deltas, float* __restrict__ xyz, float* __restrict__ dirs,
                                                             int32_t* __restrict__ ray_idx, int32_t* __restrict__ ray_count_out, int32_t* __restrict__ total,
                                                             uint8_t* __restrict__ overflow) {
  const float box[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
  if (R == 0 && blockIdx.x == 0 && threadIdx.x == 0) { *total = 0; *overflow = 0; }
  for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (long)gridDim.x * blockDim.x) {
    const float o[3] = {origin[3 * r], origin[3 * r + 1], origin[3 * r + 2]};
    const float d[3] = {dir[3 * r], dir[3 * r + 1], dir[3 * r + 2]};
    const float len = pk::dir_length(d);
    const float u[3] = {len > 0.f ? occ::div_rn(d[0], len) : 0.f, len > 0.f ? occ::div_rn(d[1], len) : 0.f, len > 0.f ? occ::div_rn(d[2], len) : 0.f};
    const float delta = occ::mul_rn(dt, len);
    const long start = ray_start[r];
    const int n = pk::march_ray(o, d, t_range[2 * r], t_range[2 * r + 1], box, bits, G, dt, k_max, [&](int i, float t, const float* p) {
      const long row = start + i;
      if (row < 0 || row >= cap) return;
      t_out[row] = t;
      deltas[row] = delta;
      xyz[3 * row] = p[0]; xyz[3 * row + 1] = p[1]; xyz[3 * row + 2] = p[2];
      dirs[3 * row] = u[0]; dirs[3 * row + 1] = u[1]; dirs[3 * row + 2] = u[2];
      ray_idx[row] = (int32_t)r;
    });
    ray_count_out[r] = pk::clamp_count((int)start, n, (int)cap);
    if (r == R - 1) {
      const long tot = start + n;
      *total = (int32_t)tot;
      *overflow = tot > cap ? 1 : 0;
    }
  }
}

// rows in [min(total, cap), cap): parked outside the box (runs behind k_packed_march_write on the same stream)
__global__ void __launch_bounds__(256) k_packed_park(const float* __restrict__ aabb, const int32_t* __restrict__ total, long cap, float* __restrict__ t_out,
                                                      float* __restrict__ deltas, float* __restrict__ xyz, float* __restrict__ dirs,
                                                      int32_t* __restrict__ ray_idx) {
  const float box[6] = {aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]};
  float p[3];
  pk::park_point(box, p);
  long first = *total;
  if (first < 0) first = 0;
  for (long row = first + (long)blockIdx.x * blockDim.x + threadIdx.x; row < cap; row += (long)gridDim.x * blockDim.x) {
    t_out[row] = 0.f;
    deltas[row] = 0.f;
    xyz[3 * row] = p[0]; xyz[3 * row + 1] = p[1]; xyz[3 * row + 2] = p[2];
    dirs[3 * row] = 0.f; dirs[3 * row + 1] = 0.f; dirs[3 * row + 2] = 1.f;
    ray_idx[row] = -1;
  }
}

// ---- compositing ----------------------------------------------------------------------------------------------------------------------
// One 64-lane wave per ray, lanes over the ray's consecutive rows (coalesced), 64 rows at a time: composite.hip's wave scan with the carry
// between the chunks, for any count.  The dense kernels hold a ray's weights in registers (D <= 256); a packed ray has no bound, so the
// forward accumulates the un-normalised sums and divides at the end, and the backward walks the ray twice.
struct RayRows {
  long s;
  int n;
};
__device__ __forceinline__ RayRows rows_of(const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count, long ray, long P) {
  const long s = ray_start[ray];
  long n = ray_count[ray];
  if (s < 0 || s >= P || n <= 0) return {0, 0};
  if (n > P - s) n = P - s;
  return {s, (int)n};
}

// (ChunkWeights / chunk_weights, a chunk's w_i and T_i from the scan of tau: packed_chunk.hpp, shared with distort.hip)

// Output channel c of a ray is accumulated by lane c (sum channels <= 64), so that the result leaves in one coalesced store.
__global__ void __launch_bounds__(256) k_packed_composite_fwd(const float* __restrict__ density, const float* __restrict__ deltas, lab4d_field_list fl,
                                                               const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count, long R, long P,
                                                               int sumC, float* __restrict__ weights, float* __restrict__ transmit,
                                                               float* __restrict__ mask, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const RayRows rr = rows_of(ray_start, ray_count, ray, P);
    float carry = 0.f, msum = 0.f, acc = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      const ChunkWeights cw = chunk_weights(density, deltas, row, live, lane, carry);
      if (live && weights) weights[row] = cw.w;
      if (live && transmit) transmit[row] = cw.T;
      msum += cw.w;
      int co = 0;
      for (int f = 0; f < fl.n_fields; ++f) {
        const int C = fl.channels[f];
        const float* v = fl.fields[f];
        if (fl.modes[f] == 2) {
          float x = 0.f;
          if (live) for (int c = 0; c < C; ++c) x += v[row * C + c];
          x = wave_sum(x);
          if (lane == co) acc += x;
          co += 1;
        } else {
          for (int c = 0; c < C; ++c) {
            const float x = wave_sum(live ? cw.w * v[row * C + c] : 0.f);
            if (lane == co + c) acc += x;
          }
          co += C;
        }
      }
    }
    msum = wave_sum(msum);
    const float inv = pk::normaliser(msum);
    float scale = 0.f;
    int co = 0;
    for (int f = 0; f < fl.n_fields; ++f) {
      const int C = fl.channels[f];
      if (fl.modes[f] == 2) {
        if (lane == co && rr.n > 0) scale = 1.f / ((float)rr.n * (float)C);
        co += 1;
      } else {
        if (lane >= co && lane < co + C) scale = inv;
        co += C;
      }
    }
    if (lane < sumC) out[ray * sumC + lane] = acc * scale;
    if (lane == 0 && mask) mask[ray] = msum;
  }
}

// dL/d(w_hat)_i of one row: the sum over the mode-0 fields of g_c v_ic
__device__ __forceinline__ float row_adjoint(const lab4d_field_list& fl, const float* __restrict__ go, long row) {
  float a = 0.f;
  int co = 0;
  for (int f = 0; f < fl.n_fields; ++f) {
    const int C = fl.channels[f];
    if (fl.modes[f] == 2) { co += 1; continue; }
    if (fl.modes[f] == 0) {
      const float* v = fl.fields[f];
      for (int c = 0; c < C; ++c) a += go[co + c] * v[row * C + c];
    }
    co += C;
  }
  return a;
}

// Pass 1 walks the ray forwards: mask = sum w and sum_i A_i w_i, which the gradient of every weight needs.  Pass 2 walks it BACKWARDS with
// the suffix scan of composite.hip's adjoint (dL/dtau_i = gw_i T_i - sum_{j>i} gw_j w_j) and a carry from the chunks behind; the prefix sum
// of tau with which a chunk starts is parked by pass 1 in the chunk's first row of g_density (or g_deltas).  That row is lane 0's own: lane 0
// alone parks the prefix, lane 0 alone reads it back in pass 2 (the other lanes get it through a shuffle), and lane 0 alone overwrites it with
// the row's gradient afterwards -- one thread's accesses to one address in program order, so nothing rests on how the hardware orders the
// memory operations of different lanes.  Without either buffer there is no tau gradient and pass 2 runs forwards.
// (g_density / g_deltas are not __restrict__: one of them is that scratch, and the compiler must keep these accesses in order.)
__global__ void __launch_bounds__(256) k_packed_composite_bwd(const float* __restrict__ density, const float* __restrict__ deltas, lab4d_field_list fl,
                                                               const int32_t* __restrict__ ray_start, const int32_t* __restrict__ ray_count, long R, long P,
                                                               int sumC, const float* __restrict__ g_mask, const float* __restrict__ g_out,
                                                               float* g_density, float* g_deltas, lab4d_field_grads gf) {
  const int lane = threadIdx.x & 63;
  float* scratch = g_density ? g_density : g_deltas;
  for (long ray = (long)blockIdx.x * 4 + (threadIdx.x >> 6); ray < R; ray += (long)gridDim.x * 4) {
    const RayRows rr = rows_of(ray_start, ray_count, ray, P);
    if (rr.n == 0) continue;
    const float gm = g_mask ? g_mask[ray] : 0.f;
    const float* go = g_out ? g_out + ray * sumC : nullptr;
    float carry = 0.f, msum = 0.f, aw = 0.f;
    for (int j0 = 0; j0 < rr.n; j0 += 64) {
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      if (scratch && lane == 0) scratch[row] = carry;
      const ChunkWeights cw = chunk_weights(density, deltas, row, live, lane, carry);
      msum += cw.w;
      if (live && go) aw += row_adjoint(fl, go, row) * cw.w;
    }
    msum = wave_sum(msum);
    aw = wave_sum(aw);
    const float inv = pk::normaliser(msum);
    const int n_chunks = (rr.n + 63) >> 6;
    float fcarry = 0.f, rcarry = 0.f;
    for (int jj = 0; jj < n_chunks; ++jj) {
      const int j0 = 64 * (scratch ? n_chunks - 1 - jj : jj);
      const bool live = j0 + lane < rr.n;
      const long row = rr.s + j0 + lane;
      float cin = fcarry;
      if (scratch) {
        const float parked = lane == 0 ? scratch[rr.s + j0] : 0.f;
        cin = __shfl(parked, 0, 64);
      }
      const ChunkWeights cw = chunk_weights(density, deltas, row, live, lane, cin);
      fcarry = cin;
      const float A = (live && go) ? row_adjoint(fl, go, row) : 0.f;
      // w_hat = w / Z:  dL/dw_i = A_i / Z - (sum_j A_j w_j) / Z^2 + g_mask
      const float gw = A * inv - aw * inv * inv + gm;
      int co = 0;
      for (int f = 0; f < fl.n_fields; ++f) {
        const int C = fl.channels[f];
        float* gv = gf.fields[f];
        if (fl.modes[f] == 2) {
          const float g = go ? go[co] / ((float)rr.n * (float)C) : 0.f;
          if (gv && live) for (int c = 0; c < C; ++c) gv[row * C + c] = g;
          co += 1;
        } else {
          if (gv && live) for (int c = 0; c < C; ++c) gv[row * C + c] = (go ? go[co + c] : 0.f) * cw.w * inv;
          co += C;
        }
      }
      if (scratch) {
        const float x = gw * cw.w;  // (0 in the lanes behind the ray: w = 0)
        const float incl = wave_rscan_incl(x, lane) + rcarry;
        float excl = __shfl_down(incl, 1, 64);
        if (lane == 63) excl = rcarry;
        rcarry = __shfl(incl, 0, 64);
        const float gtau = gw * cw.T - excl;
        if (live) {
          const float dn = density[row], dl = deltas[row];
          if (g_density) g_density[row] = gtau * dl;
          if (g_deltas) g_deltas[row] = gtau * dn;
        }
      }
    }
  }
}

}  // namespace lab4d
using namespace lab4d;

static int check_march(const char* what, int G, long R, float dt, int k_max) {
  LAB4D_REQUIRE(R >= 0, "%s: R < 0", what);
  LAB4D_REQUIRE(G >= lab4d_occ::kMinG && G <= lab4d_occ::kMaxG, "%s: G = %d outside [%d, %d]", what, G, lab4d_occ::kMinG, lab4d_occ::kMaxG);
  LAB4D_REQUIRE(dt > 0.f && lab4d_occ::finite_f(dt), "%s: dt = %g must be finite and > 0", what, (double)dt);
  LAB4D_REQUIRE(k_max >= 1, "%s: k_max = %d must be >= 1", what, k_max);
  LAB4D_REQUIRE(R * (long)k_max < (1L << 31), "%s: R * k_max = %ld * %d does not fit 31 bits", what, R, k_max);
  return LAB4D_OK;
}

extern "C" int lab4d_packed_march_count(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G,
                                        long R, float dt, int k_max, int32_t* ray_count, void* stream) {
  if (int e = check_march("packed_march_count", G, R, dt, k_max)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(origin && dir && t_range && aabb && bits && ray_count, "packed_march_count: null pointer");
  hipLaunchKernelGGL(k_packed_march_count, dim3(grid_1d(R, 256, 16384)), dim3(256), 0, (hipStream_t)stream, origin, dir, t_range, aabb, bits, G, R, dt, k_max,
                     ray_count);
  return check_launch("packed_march_count");
}

extern "C" int lab4d_packed_march_write(const float* origin, const float* dir, const float* t_range, const float* aabb, const uint32_t* bits, int G,
                                        long R, float dt, int k_max, const int32_t* ray_start, long cap, float* t, float* deltas, float* xyz,
                                        float* dirs, int32_t* ray_idx, int32_t* ray_count_out, int32_t* total, uint8_t* overflow, void* stream) {
  if (int e = check_march("packed_march_write", G, R, dt, k_max)) return e;
  LAB4D_REQUIRE(cap >= 0 && cap < (1L << 31), "packed_march_write: cap = %ld outside [0, 2^31)", cap);
  LAB4D_REQUIRE(aabb && total && overflow, "packed_march_write: null pointer");
  LAB4D_REQUIRE(R == 0 || (origin && dir && t_range && bits && ray_start && ray_count_out), "packed_march_write: null pointer");
  LAB4D_REQUIRE(cap == 0 || (t && deltas && xyz && dirs && ray_idx), "packed_march_write: null packed buffer");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_packed_march_write, dim3(grid_1d(R, 256, 16384)), dim3(256), 0, st, origin, dir, t_range, aabb, bits, G, R, dt, k_max, ray_start, cap, t,
                     deltas, xyz, dirs, ray_idx, ray_count_out, total, overflow);
  if (int e = check_launch("packed_march_write")) return e;
  if (cap == 0) return LAB4D_OK;
  hipLaunchKernelGGL(k_packed_park, dim3(grid_1d(cap, 256, 16384)), dim3(256), 0, st, aabb, total, cap, t, deltas, xyz, dirs, ray_idx);
  return check_launch("packed_march_write (park)");
}

static int check_packed_fields(const char* what, const lab4d_field_list* fl, int* sumC) {
  LAB4D_REQUIRE(fl && fl->n_fields >= 0 && fl->n_fields <= LAB4D_MAX_FIELDS, "%s: bad field list", what);
  int s = 0;
  for (int i = 0; i < fl->n_fields; ++i) {
    LAB4D_REQUIRE(fl->fields[i] && fl->channels[i] >= 1 && fl->channels[i] <= 64 && fl->modes[i] >= 0 && fl->modes[i] <= 2, "%s: bad field %d", what, i);
    s += fl->modes[i] == 2 ? 1 : fl->channels[i];
  }
  LAB4D_REQUIRE(s <= 64, "%s: %d output channels, at most 64", what, s);
  *sumC = s;
  return LAB4D_OK;
}

extern "C" int lab4d_packed_composite_forward(const float* density, const float* deltas, const lab4d_field_list* fl, const int32_t* ray_start,
                                              const int32_t* ray_count, long R, long P, float* weights, float* transmit, float* mask, float* out,
                                              void* stream) {
  LAB4D_REQUIRE(R >= 0 && R < (1L << 31) && P >= 0 && P < (1L << 31), "packed_composite_forward: R = %ld or P = %ld outside [0, 2^31)", R, P);
  int sumC = 0;
  if (int e = check_packed_fields("packed_composite_forward", fl, &sumC)) return e;
  if (R == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start && ray_count, "packed_composite_forward: null ray_start / ray_count");
  LAB4D_REQUIRE(P == 0 || (density && deltas), "packed_composite_forward: null density / deltas");
  LAB4D_REQUIRE(sumC == 0 || out, "packed_composite_forward: out is null");
  hipLaunchKernelGGL(k_packed_composite_fwd, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, density, deltas, *fl, ray_start, ray_count, R, P, sumC,
                     weights, transmit, mask, out);
  return check_launch("packed_composite_forward");
}

extern "C" int lab4d_packed_composite_backward(const float* density, const float* deltas, const lab4d_field_list* fl, const int32_t* ray_start,
                                               const int32_t* ray_count, long R, long P, const float* g_mask, const float* g_out, float* g_density,
                                               float* g_deltas, const lab4d_field_grads* g_fields, void* stream) {
  LAB4D_REQUIRE(R >= 0 && R < (1L << 31) && P >= 0 && P < (1L << 31), "packed_composite_backward: R = %ld or P = %ld outside [0, 2^31)", R, P);
  int sumC = 0;
  if (int e = check_packed_fields("packed_composite_backward", fl, &sumC)) return e;
  LAB4D_REQUIRE(g_fields && g_fields->n_fields == fl->n_fields, "packed_composite_backward: g_fields does not match the field list");
  if (R == 0 || P == 0) return LAB4D_OK;
  LAB4D_REQUIRE(ray_start && ray_count && density && deltas, "packed_composite_backward: null pointer");
  hipLaunchKernelGGL(k_packed_composite_bwd, dim3(grid_1d(R, 4, 16384)), dim3(256), 0, (hipStream_t)stream, density, deltas, *fl, ray_start, ray_count, R, P, sumC,
                     g_mask, g_out, g_density, g_deltas, *g_fields);
  return check_launch("packed_composite_backward");
}
