// CPU twin of lab4d_amd/csrc/hashsdf.hip: serial loops over the SAME functions (csrc/hashsdf_math.hpp) with the layout of
// include/lab4d_hashsdf.h, the adjoint in the kernel's order (workgroup b takes the tiles b, b + n_rows, ...; one partial row per
// workgroup; rows folded ascending).  Built by tests/host_twin.py with g++ -ffp-contract=off; tests/test_hashsdf_host.py holds it to
// float64 autograd over oracle/hashgrid_oracle.py.  Returns 0, or -1 for sizes outside the contract.
#include <stdint.h>

#include <vector>

#include "hashsdf_math.hpp"

namespace hs = lab4d_hsdf;

static bool sizes_ok(long S, int L, int log2_T, int F) {
  return S >= 0 && L >= 1 && L <= 32 && F >= 1 && F <= 8 && L * F == hs::kEnc && log2_T >= 4 && log2_T <= 24;
}

template <int F>
static void forward_t(const float* x01, const float* table, const int32_t* res, long S, int log2_T, const float* W1, const float* b1, const float* w2,
                      const float* b2, float* sdf, float* grad01) {
  for (long s = 0; s < S; ++s) {
    float g[3];
    hs::sample_forward<F>(x01 + 3 * s, table, res, log2_T, W1, b1, w2, b2[0], sdf + s, g);
    if (grad01)
      for (int a = 0; a < 3; ++a) grad01[3 * s + a] = g[a];
  }
}

template <int F>
static void backward_t(const float* x01, const float* table, const int32_t* res, long S, int log2_T, const float* W1, const float* b1, const float* w2,
                       const float* g_sdf, const float* g_grad01, float* g_table, float* g_W1, float* g_b1, float* g_w2, float* g_b2, int n_rows) {
  const bool dense = g_W1 || g_b1 || g_w2 || g_b2;
  const long tiles = (S + hs::kTile - 1) / hs::kTile;
  long grid = tiles < n_rows ? tiles : n_rows;
  std::vector<float> work((size_t)(grid > 0 ? grid : 1) * hs::kRow, 0.f);
  for (long blk = 0; blk < grid; ++blk) {
    std::vector<float> A(hs::kHid * hs::kEnc, 0.f), B(hs::kHid, 0.f);
    float accS = 0.f;
    for (long tile = blk; tile < tiles; tile += grid) {
      const long s1 = (tile + 1) * hs::kTile < S ? (tile + 1) * hs::kTile : S;
      for (long s = tile * hs::kTile; s < s1; ++s) {
        const float* p = x01 + 3 * s;
        const float gs = g_sdf ? g_sdf[s] : 0.f;
        float ct[3] = {0.f, 0.f, 0.f};
        if (g_grad01)
          for (int a = 0; a < 3; ++a) ct[a] = g_grad01[3 * s + a];
        const bool in = hs::inside_box(p);
        float enc[hs::kEnc], e[hs::kEnc], v[hs::kEnc];
        if (in) {
          hs::gather_enc<F>(p, table, res, log2_T, gs, ct, enc, e);
        } else {
          for (int k = 0; k < hs::kEnc; ++k) enc[k] = 0.f, e[k] = 0.f;
        }
        uint64_t m;
        hs::hidden(enc, W1, b1, w2, 0.f, &m, v);
        const bool active = in && (gs != 0.f || ct[0] != 0.f || ct[1] != 0.f || ct[2] != 0.f);
        if (g_table && active) hs::table_adjoint<F, false>(p, res, log2_T, gs, ct, v, true, g_table, 0);
        for (int t = 0; t < hs::kTile; ++t) {  // lane t of the workgroup: row t / 4, columns (t % 4) * 8 ..; B[j] as its lane with t % 4 == 0 holds it
          float other = 0.f;
          hs::dense_visit(m, t >> 2, e + (t & 3) * 8, gs, A.data() + (t >> 2) * hs::kEnc + (t & 3) * 8, (t & 3) == 0 ? &B[t >> 2] : &other);
        }
        accS += gs;
      }
    }
    float* row = work.data() + blk * hs::kRow;
    for (int j = 0; j < hs::kHid; ++j) {
      const float Bj = B[j];
      float q[4];
      for (int kq = 0; kq < 4; ++kq) {
        for (int i = 0; i < 8; ++i) row[j * hs::kEnc + kq * 8 + i] = w2[j] * A[j * hs::kEnc + kq * 8 + i];
        q[kq] = hs::dense_dw2_share(W1 + j * hs::kEnc + kq * 8, A.data() + j * hs::kEnc + kq * 8);
      }
      row[hs::kHid * hs::kEnc + j] = w2[j] * Bj;
      row[hs::kHid * hs::kEnc + hs::kHid + j] = ((q[0] + q[1]) + (q[2] + q[3])) + b1[j] * Bj;
    }
    row[hs::kRow - 1] = accS;
  }
  if (!dense) return;
  for (int i = 0; i < hs::kRow; ++i) {
    float s = 0.f;
    for (long r = 0; r < grid; ++r) s += work[r * hs::kRow + i];
    const int o1 = hs::kHid * hs::kEnc, o2 = o1 + hs::kHid, o3 = o2 + hs::kHid;
    if (i < o1) { if (g_W1) g_W1[i] = s; }
    else if (i < o2) { if (g_b1) g_b1[i - o1] = s; }
    else if (i < o3) { if (g_w2) g_w2[i - o2] = s; }
    else if (g_b2) g_b2[0] = s;
  }
}

extern "C" int hashsdf_host_forward(const float* x01, const float* table, const int32_t* res, long S, int L, int log2_T, int F, const float* W1,
                                    const float* b1, const float* w2, const float* b2, float* sdf, float* grad01) {
  if (!sizes_ok(S, L, log2_T, F)) return -1;
  if (F == 1) forward_t<1>(x01, table, res, S, log2_T, W1, b1, w2, b2, sdf, grad01);
  else if (F == 2) forward_t<2>(x01, table, res, S, log2_T, W1, b1, w2, b2, sdf, grad01);
  else if (F == 4) forward_t<4>(x01, table, res, S, log2_T, W1, b1, w2, b2, sdf, grad01);
  else forward_t<8>(x01, table, res, S, log2_T, W1, b1, w2, b2, sdf, grad01);
  return 0;
}

// g_table is accumulated into (the caller zero-fills it); g_W1, g_b1, g_w2, g_b2 are written; any of them, g_sdf or g_grad01 may be null
extern "C" int hashsdf_host_backward(const float* x01, const float* table, const int32_t* res, long S, int L, int log2_T, int F, const float* W1,
                                     const float* b1, const float* w2, const float* g_sdf, const float* g_grad01, float* g_table, float* g_W1, float* g_b1,
                                     float* g_w2, float* g_b2, int n_rows) {
  if (!sizes_ok(S, L, log2_T, F) || n_rows < 1 || n_rows > hs::kMaxRows) return -1;
  if (F == 1) backward_t<1>(x01, table, res, S, log2_T, W1, b1, w2, g_sdf, g_grad01, g_table, g_W1, g_b1, g_w2, g_b2, n_rows);
  else if (F == 2) backward_t<2>(x01, table, res, S, log2_T, W1, b1, w2, g_sdf, g_grad01, g_table, g_W1, g_b1, g_w2, g_b2, n_rows);
  else if (F == 4) backward_t<4>(x01, table, res, S, log2_T, W1, b1, w2, g_sdf, g_grad01, g_table, g_W1, g_b1, g_w2, g_b2, n_rows);
  else backward_t<8>(x01, table, res, S, log2_T, W1, b1, w2, g_sdf, g_grad01, g_table, g_W1, g_b1, g_w2, g_b2, n_rows);
  return 0;
}
