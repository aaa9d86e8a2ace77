// The hash field's SDF with its gradient in the point, and the adjoint of both (second-order terms included), fused: encoding, the
// 32 -> 64 -> 1 geometry net and the chain rule through both in one kernel each way.  Contract: include/lab4d_hashsdf.h; every rule and
// all of the arithmetic: hashsdf_math.hpp, shared with the CPU twin tests/host_harness/hashsdf_host.cpp.  Gather-bound like the encoding
// itself (hashgrid.hip): no MFMA.  The table gradient goes through fp32 atomics (wave_run_add); the dense gradients through per-workgroup
// partial rows folded in order: no atomics on them, no read-back, no allocation -- the calls can be captured in a hipGraph.
#include "common.hpp"
#include "hashsdf_math.hpp"

namespace lab4d {
namespace hs = lab4d_hsdf;

// W1 | b1 | w2 into LDS (8.5 KB); every lane then reads the same address at the same time: a broadcast, no bank conflict
__device__ __forceinline__ void load_net(const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ w2, float* s_W1, float* s_b1,
                                         float* s_w2) {
  for (int i = threadIdx.x; i < hs::kHid * hs::kEnc; i += blockDim.x) s_W1[i] = W1[i];
  if (threadIdx.x < hs::kHid) s_b1[threadIdx.x] = b1[threadIdx.x], s_w2[threadIdx.x] = w2[threadIdx.x];
  __syncthreads();
}

// Per level the walks need some eight scalars that do not change from one sample to the next (resolution, dense-or-hashed, slab bases).  Hoisted out of
// the sample loop for all L levels they spill the scalar registers; the loop body takes the two values they derive from through this, and recomputes.
__device__ __forceinline__ void per_iteration(const int*& res, int& log2_T) { asm volatile("" : "+s"(res), "+s"(log2_T)); }

// One lane per sample, grid-stride.  enc and v live in registers (32 + 32), z is formed a row at a time, the table is gathered a second
// time for grad01 instead of keeping the 96 Jacobian entries.
template <int F>
__global__ void __launch_bounds__(hs::kTile, 3) k_hashsdf_fwd(const float* __restrict__ x, const float* __restrict__ table, const int* __restrict__ res_, long S,
                                                            int log2_T_, const float* __restrict__ W1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ sdf,
                                                            float* __restrict__ grad01) {
  __shared__ float s_W1[hs::kHid * hs::kEnc], s_b1[hs::kHid], s_w2[hs::kHid];
  load_net(W1, b1, w2, s_W1, s_b1, s_w2);
  const float bias2 = b2[0];
  for (long s = (long)blockIdx.x * blockDim.x + threadIdx.x; s < S; s += (long)gridDim.x * blockDim.x) {
    const int* res = res_;
    int log2_T = log2_T_;
    per_iteration(res, log2_T);
    const float p[3] = {x[3 * s], x[3 * s + 1], x[3 * s + 2]};
    float d, g[3];
    hs::sample_forward<F>(p, table, res, log2_T, s_W1, s_b1, s_w2, bias2, &d, g);
    sdf[s] = d;
    if (grad01) grad01[3 * s] = g[0], grad01[3 * s + 1] = g[1], grad01[3 * s + 2] = g[2];
  }
}

// Resident grid: workgroup b takes the tiles b, b + gridDim.x, ... of 256 samples.  The trip count is wave-uniform and lanes past the end
// carry zeros (as in k_hashgrid_bwd): the table updates are combined across the lanes of a wave.  Per tile the lanes park e (32 floats), the
// mask word and gs in LDS; then lane t adds the tile's samples into its 8 entries of A (row t / 4, columns (t % 4) * 8 ..) and its B, held in
// registers across all tiles.  At the end the workgroup writes ONE partial row {dW1, db1, dw2, db2} to work[blockIdx.x].  work == nullptr:
// the table gradient alone; g_table == nullptr: the dense gradients alone.
template <int F>
__global__ void __launch_bounds__(hs::kTile, 3) k_hashsdf_bwd(const float* __restrict__ x, const float* __restrict__ table, const int* __restrict__ res_, long S,
                                                            int log2_T_, const float* __restrict__ W1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ g_sdf,
                                                            const float* __restrict__ g_grad01, float* __restrict__ g_table, float* __restrict__ work) {
  __shared__ float s_W1[hs::kHid * hs::kEnc], s_b1[hs::kHid], s_w2[hs::kHid];
  __shared__ float4 s_e[8 * hs::kTile];  // [quad i of the 32 floats][sample]: consecutive lanes write consecutive 16 bytes
  __shared__ uint64_t s_mask[hs::kTile];
  __shared__ float s_gs[hs::kTile];
  load_net(W1, b1, w2, s_W1, s_b1, s_w2);
  const int t = threadIdx.x, lane = t & 63, j = t >> 2, kq = t & 3;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, accB = 0.f, accS = 0.f;
  const long tiles = (S + hs::kTile - 1) / hs::kTile;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int* res = res_;
    int log2_T = log2_T_;
    per_iteration(res, log2_T);
    const long s0 = tile * hs::kTile, s = s0 + t;
    const bool live = s < S;
    const long sc = live ? s : S - 1;
    const float p[3] = {x[3 * sc], x[3 * sc + 1], x[3 * sc + 2]};
    const float gs = (live && g_sdf) ? g_sdf[s] : 0.f;
    float ct[3] = {0.f, 0.f, 0.f};
    if (live && g_grad01) ct[0] = g_grad01[3 * s], ct[1] = g_grad01[3 * s + 1], ct[2] = g_grad01[3 * s + 2];
    const bool in = live && hs::inside_box(p);
    float enc[hs::kEnc], e[hs::kEnc], v[hs::kEnc];
    if (in) {
      hs::gather_enc<F>(p, table, res, log2_T, gs, ct, enc, e);
    } else {
#pragma unroll
      for (int k = 0; k < hs::kEnc; ++k) enc[k] = 0.f, e[k] = 0.f;
    }
    if (work) {
#pragma unroll
      for (int i = 0; i < 8; ++i) s_e[i * hs::kTile + t] = make_float4(e[4 * i], e[4 * i + 1], e[4 * i + 2], e[4 * i + 3]);
      s_gs[t] = gs;
    }
    uint64_t m;
    hs::hidden(enc, s_W1, s_b1, s_w2, 0.f, &m, v);
    if (work) s_mask[t] = m;
    if (g_table) {
      const bool active = in && (gs != 0.f || ct[0] != 0.f || ct[1] != 0.f || ct[2] != 0.f);
      if (__any(active)) hs::table_adjoint<F, true>(p, res, log2_T, gs, ct, v, active, g_table, lane);  // (wave-uniform)
    }
    if (work) {  // (uniform over the grid)
      __syncthreads();
      const int n_tile = (int)(S - s0 < hs::kTile ? S - s0 : hs::kTile);
      for (int i = 0; i < n_tile; ++i) {
        const float4 a = s_e[(2 * kq) * hs::kTile + i], b = s_e[(2 * kq + 1) * hs::kTile + i];
        const float e8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        const float g = s_gs[i];
        hs::dense_visit(s_mask[i], j, e8, g, acc, &accB);
        accS += g;
      }
      __syncthreads();
    }
  }
  if (!work) return;
  float* row = work + (size_t)blockIdx.x * hs::kRow;
  const float wj = s_w2[j];
#pragma unroll
  for (int i = 0; i < 8; ++i) row[j * hs::kEnc + kq * 8 + i] = wj * acc[i];
  float share = hs::dense_dw2_share(s_W1 + j * hs::kEnc + kq * 8, acc);
  share += __shfl_xor(share, 1, 64);
  share += __shfl_xor(share, 2, 64);
  if (kq == 0) {
    row[hs::kHid * hs::kEnc + j] = wj * accB;
    row[hs::kHid * hs::kEnc + hs::kHid + j] = share + s_b1[j] * accB;
  }
  if (t == 0) row[hs::kRow - 1] = accS;
}

// One lane per dense entry: the partial rows folded in ascending workgroup order.
__global__ void __launch_bounds__(256) k_hashsdf_reduce(const float* __restrict__ work, int n_rows, float* __restrict__ g_W1, float* __restrict__ g_b1,
                                                         float* __restrict__ g_w2, float* __restrict__ g_b2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= hs::kRow) return;
  float s = 0.f;
  for (int r = 0; r < n_rows; ++r) s += work[(size_t)r * hs::kRow + i];
  constexpr int o1 = hs::kHid * hs::kEnc, o2 = o1 + hs::kHid, o3 = o2 + hs::kHid;
  if (i < o1) { if (g_W1) g_W1[i] = s; }
  else if (i < o2) { if (g_b1) g_b1[i - o1] = s; }
  else if (i < o3) { if (g_w2) g_w2[i - o2] = s; }
  else if (g_b2) g_b2[0] = s;
}

}  // namespace lab4d
using namespace lab4d;

#define HASHSDF_CHECKS(name)                                                                                                                     \
  LAB4D_REQUIRE(S >= 0, name ": S = %d is negative", S);                                                                                         \
  LAB4D_REQUIRE(L >= 1 && L <= 32 && F >= 1 && F <= 8 && L * F == lab4d_hsdf::kEnc,                                                              \
                name ": L = %d, F = %d: the geometry net is instantiated for L * F = 32 hash features (L <= 32, F <= 8)", L, F);                  \
  LAB4D_REQUIRE(log2_T >= 4 && log2_T <= 24, name ": log2_T = %d outside [4, 24]", log2_T);                                                      \
  LAB4D_REQUIRE(x01 && table && res, name ": null pointer (x01, table, res)");                                                                   \
  LAB4D_REQUIRE(W1 && b1 && w2 && b2, name ": null pointer (W1, b1, w2, b2)");

static_assert(lab4d_hsdf::kMaxRows == LAB4D_HASHSDF_WORK_ROWS, "hashsdf_math.hpp and lab4d_hashsdf.h disagree on the resident grid");

extern "C" int lab4d_hashsdf_forward(const float* x01, const float* table, const int32_t* res, int S, int L, int log2_T, int F, const float* W1,
                                     const float* b1, const float* w2, const float* b2, float* sdf, float* grad01, void* stream) {
  HASHSDF_CHECKS("hashsdf_forward");
  LAB4D_REQUIRE(sdf, "hashsdf_forward: null pointer (sdf)");
  if (S == 0) return LAB4D_OK;
  long g = (S + (long)hs::kTile - 1) / hs::kTile;
  if (g > 2048) g = 2048;
#define LAUNCH_FWD(FF)                                                                                                                          \
  hipLaunchKernelGGL(k_hashsdf_fwd<FF>, dim3((unsigned)g), dim3(hs::kTile), 0, (hipStream_t)stream, x01, table, res, (long)S, log2_T, W1, b1, w2, b2, sdf, \
                     grad01)
  if (F == 1) LAUNCH_FWD(1);
  else if (F == 2) LAUNCH_FWD(2);
  else if (F == 4) LAUNCH_FWD(4);
  else LAUNCH_FWD(8);
#undef LAUNCH_FWD
  return check_launch("hashsdf_forward");
}

extern "C" int lab4d_hashsdf_backward(const float* x01, const float* table, const int32_t* res, int S, int L, int log2_T, int F, const float* W1,
                                      const float* b1, const float* w2, const float* b2, const float* g_sdf, const float* g_grad01, float* g_table,
                                      float* g_W1, float* g_b1, float* g_w2, float* g_b2, float* work, int n_work_rows, void* stream) {
  HASHSDF_CHECKS("hashsdf_backward");
  const bool dense = g_W1 || g_b1 || g_w2 || g_b2;
  LAB4D_REQUIRE(g_sdf || g_grad01, "hashsdf_backward: null pointer (g_sdf and g_grad01: at least one cotangent)");
  LAB4D_REQUIRE(g_table || dense, "hashsdf_backward: null pointer (no gradient asked for)");
  LAB4D_REQUIRE(!dense || (work && n_work_rows >= 1 && n_work_rows <= hs::kMaxRows),
                "hashsdf_backward: the dense gradients need a work buffer of n_work_rows x %d floats with n_work_rows in [1, %d], got %s, n_work_rows = %d",
                hs::kRow, hs::kMaxRows, work ? "a buffer" : "NULL", n_work_rows);
  hipStream_t st = (hipStream_t)stream;
  long g = (S + (long)hs::kTile - 1) / hs::kTile;  // tiles
  const long cap = dense ? n_work_rows : hs::kMaxRows;
  if (g > cap) g = cap;
  if (g > 0) {
    float* wk = dense ? work : nullptr;
#define LAUNCH_BWD(FF)                                                                                                                          \
  hipLaunchKernelGGL(k_hashsdf_bwd<FF>, dim3((unsigned)g), dim3(hs::kTile), 0, st, x01, table, res, (long)S, log2_T, W1, b1, w2, g_sdf, g_grad01, g_table, wk)
    if (F == 1) LAUNCH_BWD(1);
    else if (F == 2) LAUNCH_BWD(2);
    else if (F == 4) LAUNCH_BWD(4);
    else LAUNCH_BWD(8);
#undef LAUNCH_BWD
    if (int e = check_launch("hashsdf_backward")) return e;
  }
  if (dense) {  // (S == 0: no rows, the dense gradients are written as zeros)
    hipLaunchKernelGGL(k_hashsdf_reduce, dim3((hs::kRow + 255) / 256), dim3(256), 0, st, (const float*)work, (int)g, g_W1, g_b1, g_w2, g_b2);
    return check_launch("hashsdf_backward (reduce)");
  }
  return LAB4D_OK;
}
