/*
 * lab4d_hashsdf.h -- the hash field's SDF with its gradient in the point, and the adjoint of both (included by lab4d_hip.h).
 *
 * What the positional-encoding fields get from compute_gradient(..., create_graph=True) (utils/torch_utils.py:4-27) for the eikonal term
 * and the normals (nnutils/nerf.py:416-493), for the field on the hash encoding (lab4d_hashgrid.h), whose encoding has no double
 * backward.  The geometry net is  enc (L * F = 32) -> 64, ReLU -> row 0 of the 16 x 64 head,  small enough for a closed form of the
 * gradient and of its adjoint, second-order terms included.  The reference has no hash field: parity is unpinned, the truth of the tests
 * is float64 autograd over oracle/hashgrid_oracle.py.  The arithmetic is lab4d_amd/csrc/hashsdf_math.hpp, shared with the CPU twin
 * tests/host_harness/hashsdf_host.cpp.  fp32, box coordinates x01 throughout.
 *
 * Rules (W1 (64,32), b1 (64): the first Linear; w2 (64), b2 (1): row 0 of the head; per level l: cell_of -> cell and position, corner c
 * with tri-linear weight wt_c and partials dwt_c[a]; T the table (L, 2^log2_T, F); res (L) int32 the levels' resolutions, each >= 1):
 *   FORWARD   inside [0,1]^3 (x >= 0 && x <= 1 on every axis; NaN is outside):
 *               enc[l,f] = sum_c wt_c T[l,v_c,f];  z = W1 enc + b1;  m = z > 0;  sdf = w2 . relu(z) + b2;  v = W1^T (m * w2);
 *               grad01[a] = sum_l res_l sum_c dwt_c[a] sum_f T[l,v_c,f] v[l,f]
 *             the derivative of the cell that cell_of picks: one-sided on a face, x01 == 1 lies in the last cell.
 *   OUTSIDE   enc = 0: sdf = w2 . relu(b1) + b2, grad01 = 0; the table is never read.
 *   ADJOINT   cotangents gs on sdf and ct (3) on grad01; coef_c = gs wt_c + res_l (dwt_c . ct); e[l,f] = sum_c coef_c T[l,v_c,f]
 *             ( = gs enc + u, u = res_l sum_c (dwt_c . ct) T );  q = m * w2;  r = W1 u:
 *               dW1 = sum q (x) e;  db1 = sum gs q;  dw2 = sum gs relu(z) + m * r;  db2 = sum gs;  dT[l,v_c,f] += coef_c v[l,f]
 *             Outside the box only the gs terms of b1, w2, b2 exist.  No gradient to the point.
 *   OUTPUTS   g_table is ACCUMULATED into with fp32 atomics (the caller zero-fills it; runs of equal vertices inside a wave are combined
 *             first, a zero update issues no atomic): its last bits depend on the order of arrival.  g_W1 (64,32), g_b1 (64), g_w2 (64),
 *             g_b2 (1) are WRITTEN: every workgroup of a resident grid of min(ceil(S / 256), n_work_rows) workgroups sums its samples in
 *             registers and writes one partial row of 2048 + 64 + 64 + 1 floats into `work`; a second kernel folds the rows in ascending
 *             order.  Deterministic for a given n_work_rows.
 *   NULLS     g_sdf or g_grad01 NULL: that cotangent is zero (not both).  g_table NULL: no table gradient.  Each of g_W1, g_b1, g_w2,
 *             g_b2 may be NULL; all four NULL: `work` is not used and may be NULL.  grad01 of the forward may be NULL.
 *   WORK      n_work_rows x 2177 floats, 1 <= n_work_rows <= LAB4D_HASHSDF_WORK_ROWS (512).
 *
 * No atomics on the dense gradients, no read-back, no allocation: capturable in a hipGraph.  Arguments are checked before any launch:
 * L * F == 32, L <= 32, F <= 8 (F is 1, 2, 4 or 8), 4 <= log2_T <= 24, the pointers above, the work buffer.
 */
#ifndef LAB4D_HASHSDF_H
#define LAB4D_HASHSDF_H

/* the largest resident grid of the adjoint = the largest n_work_rows (a constant, not an entry point: tests/test_abi.py pins the set of
 * host-only entry points) */
#define LAB4D_HASHSDF_WORK_ROWS 512

/* x01 (S,3), table (L, 2^log2_T, F), res (L) int32 -> sdf (S), grad01 (S,3) or NULL.  One lane per sample. */
int lab4d_hashsdf_forward(const float* x01, const float* table, const int32_t* res, int S, int L, int log2_T, int F, const float* W1,
                          const float* b1, const float* w2, const float* b2, float* sdf, float* grad01, void* stream);

/* g_sdf (S), g_grad01 (S,3) -> g_table (L, 2^log2_T, F) accumulated; g_W1, g_b1, g_w2, g_b2 written. */
int lab4d_hashsdf_backward(const float* x01, const float* table, const int32_t* res, int S, int L, int log2_T, int F, const float* W1,
                           const float* b1, const float* w2, const float* b2, const float* g_sdf, const float* g_grad01, float* g_table,
                           float* g_W1, float* g_b1, float* g_w2, float* g_b2, float* work, int n_work_rows, void* stream);

#endif /* LAB4D_HASHSDF_H */
