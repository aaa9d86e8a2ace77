// The hash field's SDF, its gradient in the point and the adjoint of both, in closed form, one sample at a time.  Contract:
// include/lab4d_hashsdf.h.  Plain C++ (LAB4D_HD convention) on top of hashgrid_math.hpp: the kernels of hashsdf.hip and the CPU twin
// tests/host_harness/hashsdf_host.cpp call the same functions.  Everything works in box coordinates x01, in fp32.
//
// The geometry net is  enc (32) -> 64, ReLU -> row 0 of the 16 x 64 head.  W1 (64 x 32), b1 (64): its first Linear; w2 (64), b2: row 0 of
// the head.  At level l, cell_of gives the cell i0 and the position w in it; corner c has the tri-linear weight wt_c and the partials
// dwt_c[a] = +-1 * (the other two factors), as in lab4d_hash::encode_level_bwd; T is the table, res_l the level's resolution.
//
// FORWARD, a point inside [0,1]^3 (the test of k_hashgrid_fwd<true>: NaN is outside):
//   enc[l,f] = sum_c wt_c T[l,v_c,f]         z = W1 enc + b1         m = z > 0         sdf = w2 . relu(z) + b2
//   q = m * w2                               v = W1^T q  (32)
//   grad01[a] = sum_l res_l sum_c dwt_c[a] sum_f T[l,v_c,f] v[l,f]
//   The derivative is the one of the cell that cell_of picks: one-sided on a face, x01 == 1 lies in the last cell.
// OUTSIDE the box: enc = 0, sdf = w2 . relu(b1) + b2 (what hashfield.forward(get_density=False) returns there), grad01 = 0; the table
// is never read.
//
// ADJOINT for the cotangents gs (on sdf) and ct (3, on grad01).  With coef_c = gs wt_c + res_l (dwt_c . ct):
//   u[l,f] = res_l sum_c (dwt_c . ct) T[l,v_c,f]         e = gs enc + u   ( = sum_c coef_c T[l,v_c,f]: formed in that one sum )
//   r = W1 u
//   dW1 += q (x) e          db1 += gs q          dw2 += gs relu(z) + m * r          db2 += gs
//   dT[l,v_c,f] += coef_c v[l,f]
//   Over a set of samples, with A[j,k] = sum_s m_sj e_sk and B[j] = sum_s m_sj gs_s (relu(z_j) = m_j (W1_j . enc + b1_j), r_j = W1_j . u):
//   dW1[j,k] = w2_j A[j,k]      db1[j] = w2_j B[j]      dw2[j] = W1_j . A[j,:] + b1_j B[j]      db2 = sum_s gs_s
//   which is how the kernel and the twin accumulate them (A and B per workgroup, the products once at its end).
//   Outside the box e = 0: only the gs terms of b1, w2 and b2 remain.  There is no gradient to the point (second derivatives in x are
//   out of scope).
#pragma once
#include "hashgrid_math.hpp"

// The level loops below are unrolled: enc, e and v are register arrays with constant indices.  Two things then have to be said to the
// compiler.  (1) Left alone it sinks a level's arithmetic down to where enc is first used, behind the gathers of ALL levels: every loaded
// table entry and every corner weight stays live (8 L F + 5 * 8 L values; 256 VGPRs, as many AGPR copies, one wave per SIMD, spills at
// F = 1).  A level's results are therefore pinned where the level ends.  (2) The table is walked twice per sample (enc, then grad01 or
// the table adjoint) with the dense layer in between; the second walk must RECOMPUTE cells, weights and addresses instead of carrying
// them across the dense layer, so the point is made opaque between the walks.  Both are lab4d_rn::pin (hd_math.hpp; nothing on the host).
#define LAB4D_OPAQUE3(y) do { lab4d_rn::pin((y)[0]); lab4d_rn::pin((y)[1]); lab4d_rn::pin((y)[2]); } while (0)

namespace lab4d_hsdf {
using lab4d_rn::pin;

constexpr int kEnc = 32;                              // L * F, the width the geometry net is instantiated for
constexpr int kHid = 64;
constexpr int kTile = 256;                            // samples per tile of the adjoint = lanes per workgroup
constexpr int kRow = kHid * kEnc + kHid + kHid + 1;   // one partial row of the dense gradients: dW1 | db1 | dw2 | db2
constexpr int kMaxRows = 512;                         // the resident grid of the adjoint: at most two workgroups per compute unit

LAB4D_HD bool inside_box(const float* p) { return p[0] >= 0.f && p[0] <= 1.f && p[1] >= 0.f && p[1] <= 1.f && p[2] >= 0.f && p[2] <= 1.f; }

struct Corner {
  uint32_t v;    // vertex index in the level's slab
  float wt;      // tri-linear weight
  float dwt[3];  // its partials in w (multiply by res for x01)
};

LAB4D_HD Corner corner_of(const uint32_t* i0, const float* w, int c, int res, int log2_T) {
  const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
  const float wx = dx ? w[0] : 1.f - w[0], wy = dy ? w[1] : 1.f - w[1], wz = dz ? w[2] : 1.f - w[2];
  Corner k;
  k.v = lab4d_hash::vertex_index(i0[0] + dx, i0[1] + dy, i0[2] + dz, res, log2_T);
  k.wt = wx * wy * wz;
  k.dwt[0] = (dx ? 1.f : -1.f) * wy * wz;
  k.dwt[1] = wx * (dy ? 1.f : -1.f) * wz;
  k.dwt[2] = wx * wy * (dz ? 1.f : -1.f);
  return k;
}

LAB4D_HD float corner_coef(const Corner& k, float gs, const float* ct, float resf) {
  return gs * k.wt + resf * (k.dwt[0] * ct[0] + k.dwt[1] * ct[1] + k.dwt[2] * ct[2]);
}

// enc (32) of a point inside the box; with e != nullptr also e = sum_c coef_c T (32)
template <int F>
LAB4D_HD void gather_enc(const float* x, const float* table, const int* res, int log2_T, float gs, const float* ct, float* enc, float* e) {
  constexpr int L = kEnc / F;
  const size_t slab = ((size_t)1 << log2_T) * F;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int r = res[l];
    uint32_t i0[3];
    float w[3], a[F], b[F];
    lab4d_hash::cell_of(x, r, i0, w);
#pragma unroll
    for (int f = 0; f < F; ++f) a[f] = 0.f, b[f] = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const Corner k = corner_of(i0, w, c, r, log2_T);
      const float* t = table + l * slab + (size_t)k.v * F;
      const float co = e ? corner_coef(k, gs, ct, (float)r) : 0.f;
#pragma unroll
      for (int f = 0; f < F; ++f) {
        const float tv = t[f];
        a[f] += k.wt * tv;
        b[f] += co * tv;
      }
    }
#pragma unroll
    for (int f = 0; f < F; ++f) {
      pin(a[f]);
      enc[l * F + f] = a[f];
      if (e) {
        pin(b[f]);
        e[l * F + f] = b[f];
      }
    }
  }
}

// z row by row; returns sdf, the 64 mask bits in *mask and v = W1^T (m * w2) in v (32)
LAB4D_HD float hidden(const float* enc, const float* W1, const float* b1, const float* w2, float b2, uint64_t* mask, float* v) {
  float sdf = b2;
  uint64_t m = 0;
#pragma unroll
  for (int k = 0; k < kEnc; ++k) v[k] = 0.f;
#pragma unroll 2  // (fully unrolled, the 2,048 LDS reads are hoisted into registers: 256 VGPRs and their AGPR copies, one wave per SIMD)
  for (int j = 0; j < kHid; ++j) {
    const float* row = W1 + j * kEnc;
    float z = b1[j];
#pragma unroll
    for (int k = 0; k < kEnc; ++k) z += row[k] * enc[k];
    const bool on = z > 0.f;
    const float q = on ? w2[j] : 0.f;
    sdf += q * z;
    m |= (uint64_t)(on ? 1 : 0) << j;
#pragma unroll
    for (int k = 0; k < kEnc; ++k) v[k] += q * row[k];
  }
  *mask = m;
  return sdf;
}

// grad01 of a point inside the box: the table gathered a second time against v
template <int F>
LAB4D_HD void gather_grad(const float* x, const float* table, const int* res, int log2_T, const float* v, float* grad01) {
  constexpr int L = kEnc / F;
  const size_t slab = ((size_t)1 << log2_T) * F;
  grad01[0] = grad01[1] = grad01[2] = 0.f;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int r = res[l];
    uint32_t i0[3];
    float w[3], acc[3] = {0.f, 0.f, 0.f};
    lab4d_hash::cell_of(x, r, i0, w);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const Corner k = corner_of(i0, w, c, r, log2_T);
      const float* t = table + l * slab + (size_t)k.v * F;
      float dot = 0.f;
#pragma unroll
      for (int f = 0; f < F; ++f) dot += t[f] * v[l * F + f];
      acc[0] += k.dwt[0] * dot;
      acc[1] += k.dwt[1] * dot;
      acc[2] += k.dwt[2] * dot;
    }
    for (int a = 0; a < 3; ++a) {
      grad01[a] += acc[a] * (float)r;
      pin(grad01[a]);
    }
  }
}

// one sample of the forward
template <int F>
LAB4D_HD void sample_forward(const float* x, const float* table, const int* res, int log2_T, const float* W1, const float* b1, const float* w2, float b2,
                             float* sdf, float* grad01) {
  float enc[kEnc], v[kEnc];
  uint64_t m;
  const bool in = inside_box(x);
  if (in) {
    gather_enc<F>(x, table, res, log2_T, 0.f, nullptr, enc, nullptr);
  } else {
#pragma unroll
    for (int k = 0; k < kEnc; ++k) enc[k] = 0.f;
  }
  *sdf = hidden(enc, W1, b1, w2, b2, &m, v);
  if (in) {
    float y[3] = {x[0], x[1], x[2]};
    LAB4D_OPAQUE3(y);
    gather_grad<F>(y, table, res, log2_T, v, grad01);
  } else {
    grad01[0] = grad01[1] = grad01[2] = 0.f;
  }
}

// dT[l,v_c,f] += coef_c v[l,f].  WAVE (device only): the whole wave calls this together, the updates go through lab4d_hash::wave_run_add
// (runs of equal vertices combined, no atomic for a zero update); a lane without a contribution passes active = false.
template <int F, bool WAVE>
LAB4D_HD void table_adjoint(const float* x0, const int* res, int log2_T, float gs, const float* ct, const float* v, bool active, float* g_table, int lane) {
  constexpr int L = kEnc / F;
  float x[3] = {x0[0], x0[1], x0[2]};
  LAB4D_OPAQUE3(x);
  const size_t slab = ((size_t)1 << log2_T) * F;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int r = res[l];
    uint32_t i0[3];
    float w[3];
    lab4d_hash::cell_of(x, r, i0, w);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const Corner k = corner_of(i0, w, c, r, log2_T);
      const float co = active ? corner_coef(k, gs, ct, (float)r) : 0.f;
      float val[lab4d_hash::MAXF];
#pragma unroll
      for (int f = 0; f < F; ++f) val[f] = co * v[l * F + f];
#if defined(__HIP_DEVICE_COMPILE__)
      if (WAVE) {
        lab4d_hash::wave_run_add(g_table + l * slab, k.v * (uint32_t)F, val, F, lane);
        continue;
      }
#endif
      for (int f = 0; f < F; ++f)
        if (val[f] != 0.f) g_table[l * slab + (size_t)k.v * F + f] += val[f];
    }
  }
}

// The dense sums are split over the 256 lanes of a workgroup: lane t owns row j = t / 4 and the 8 columns from k0 = (t % 4) * 8.
// One sample's contribution to a lane's A[j, k0 .. k0 + 8) and B[j]:
LAB4D_HD void dense_visit(uint64_t mask, int j, const float* e8, float gs, float* acc8, float* accB) {
  if ((mask >> j) & 1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) acc8[i] += e8[i];
    *accB += gs;
  }
}
// and the lane's share of W1_j . A[j,:] at the end (the four shares of a row are then added as (0 + 1) + (2 + 3))
LAB4D_HD float dense_dw2_share(const float* W1_j_k0, const float* acc8) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += W1_j_k0[i] * acc8[i];
  return s;
}

}  // namespace lab4d_hsdf
