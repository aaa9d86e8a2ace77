// Merge of two packed sample lists per ray by depth (csrc/pmerge.hip; contract: include/lab4d_pmerge.h): what MultiFields.compose_fields
// (nnutils/multifields.py:339-398) does for a foreground and a background field on the dense layout -- concatenate along the depth axis,
// z-sort per ray, gather every per-sample key through the permutation -- for two packed lists whose rays have their own lengths.  Plain
// C++ behind LAB4D_HD: the kernels run these functions one row per lane, tests/host_harness/pmerge/pmerge_host.cpp compiles them with g++ as
// serial loops, and the GPU suite holds the kernels word for word to that twin.
//
// ROWS     list A has Pa rows, list B has Pb rows, Pa + Pb < 2^31.  Ray r owns rows_of(start, count, r, P) of each list (prune_math.hpp): a
//          (start, count) that leaves [0, P) is cut to it.  na, nb: the cut counts.
// ORDER    both lists non-decreasing in t within every ray, free of NaN, t in the same units along the same ray (the caller's business:
//          the fields may live in different frames, so a merged list carries no xyz / dirs).  The merged order of a ray is the stable
//          argsort of [t_a | t_b]: a tie between the lists goes to A, the order inside a list is kept (lab4d_compose_order's rule).  As
//          ranks:  A's i-th row goes to i + #{j : t_b[j] < t_a[i]},  B's j-th row goes to j + #{i : t_a[i] <= t_b[j]}  (place_a, place_b).
//          Each count is one binary search, count_before: its loop is written once, here.  Plain fp32 < and <=: -0.0 ties with 0.0.
//          Input that breaks the precondition: unspecified, but count_before returns a value in [0, n] after at most ceil(log2(n + 1))
//          steps whatever it reads (a NaN compares false), so a place lies inside the ray's na + nb merged rows and the call terminates.
// LAYOUT   the march's and the prune's: count[r] = na + nb, start = its exclusive prefix sum (the caller's scan), total = the sum,
//          untruncated; a STATIC capacity cap: rows >= cap are not written, the emitted count is clamp_count (packed_math.hpp),
//          overflow = total > cap; rows in [min(total, cap), cap) are parked with t = deltas = 0, ray_idx = src = -1.
// PER ROW  t and deltas copied bit for bit; ray_idx = the ray; src = the source row in the concatenation (src_of: i for A's row i,
//          Pa + i for B's row i); pos_a (Pa), pos_b (Pb) = the merged row of every input row, -1 where no ray owns it or it fell behind cap.
// GATHER   out[j, :] = 0 if idx[j] < 0, a[idx[j], :] if idx[j] < Pa, b[idx[j] - Pa, :] if idx[j] < Pa + Pb, 0 behind that; a NULL part
//          reads as zeros (gather_value).  Forward idx = src; the adjoint of a part is the same call with g_out as part A and idx = pos.
#pragma once
#include "prune_math.hpp"

namespace lab4d_pmerge {
using lab4d_prune::Rows;
using lab4d_prune::rows_of;

// how many of the n ascending values v lie before x: v[k] < x, or v[k] <= x with or_equal.  The first k whose value does not.
LAB4D_HD int count_before(const float* v, int n, float x, bool or_equal) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const float m = v[mid];
    if (or_equal ? m <= x : m < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the place within its ray's merged rows of A's i-th row (t_b: the ray's nb rows of B) and of B's j-th row (t_a: the ray's na rows of A)
LAB4D_HD int place_a(int i, float t_ai, const float* t_b, int nb) { return i + count_before(t_b, nb, t_ai, false); }
LAB4D_HD int place_b(int j, float t_bj, const float* t_a, int na) { return j + count_before(t_a, na, t_bj, true); }

// the source row in the concatenation [A | B]
LAB4D_HD int32_t src_of(bool from_b, long row, long Pa) { return (int32_t)(from_b ? Pa + row : row); }

LAB4D_HD float gather_value(const float* a, long Pa, const float* b, long Pb, long idx, int C, int c) {
  if (idx < 0) return 0.f;
  if (idx < Pa) return a ? a[idx * C + c] : 0.f;
  if (idx < Pa + Pb) return b ? b[(idx - Pa) * C + c] : 0.f;
  return 0.f;
}

}  // namespace lab4d_pmerge
