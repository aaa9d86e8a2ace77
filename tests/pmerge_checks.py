"""Shared by tests/test_pmerge_host.py (CPU twin against numpy's stable argsort) and tests/test_gpu_zzzzzzzzzzzzzpmerge.py (kernels against
the twin): the host harness of the merge of two packed lists (tests/host_harness/pmerge/pmerge_host.cpp over lab4d_amd/csrc/pmerge_math.hpp),
the generator of the test lists, and the rules of include/lab4d_pmerge.h restated with numpy.  A helper module: no test in it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_twin  # noqa: E402

TWIN = "pmerge/pmerge"  # tests/host_harness/pmerge/pmerge_host.cpp: a folder of its own (tests/test_host_twin.py pins the census of the twins beside it)
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 200)
# (na, nb) of the first rays: every combination of empty (0) / shorter than a wave (1, 2, 63) / across a 64-row chunk (64, 65, 129, 200), then
# sums that land on and around 64 and 128: 64, 65, 127, 128, 129
PAIRS = ((0, 0), (0, 2), (0, 65), (1, 0), (63, 1), (2, 129), (64, 0), (65, 63), (200, 129), (1, 63), (63, 2), (63, 64), (63, 65), (64, 65), (129, 200), (2, 2))
PAD = 5  # rows behind the capacity in every merged buffer: they must keep their sentinel
SENTINEL_F, SENTINEL_I = np.float32(-7.5), np.int32(-7)
MERGED_F, MERGED_I = ("t", "deltas"), ("ray_idx", "src")


def build_host():
    os.makedirs(os.path.join(host_twin.BUILD, os.path.dirname(TWIN)), exist_ok=True)  # (host_twin makes its build folder, not one below it)
    return host_twin.load(TWIN)


def _layout(rng, lengths, gaps):
    gap = (rng.integers(0, 3, len(lengths)) == 0) * rng.integers(1, 4, len(lengths)) if gaps else np.zeros(len(lengths), np.int64)
    start = np.cumsum(lengths + gap) - lengths
    return start.astype(np.int32), lengths.astype(np.int32), int((lengths + gap).sum())


def make_pair(R, seed, gaps=True):
    """Two packed lists of the same R rays.  Lengths (na, nb): PAIRS for the first rays, then drawn from LENGTHS.  Gaps of 1..3 unowned rows
    in front of a third of the rays, in each list on its own.  t per ray sorted from the lattice k / 64 with k below about half the ray's
    rows of both lists, so that ties between the lists and repeats inside a list are frequent; a zero is -0.0 half of the time.  From the
    end: the last ray owns (P - 5, 65) of A and (P - 3, 40) of B, which leave [0, P) and are cut to 5 and 3 rows (R = 1: that ray alone);
    with R >= 3 the ray before it has the SAME 65 values in both lists and the one before that has all 64 rows of A behind all 63 of B;
    with R >= 5 the ray before those starts at -3 in A (no rows) and has 2 rows in B.  numpy float32 / int32."""
    rng = np.random.default_rng(seed)
    n_special = min(R, 1) + (2 if R >= 3 else 0) + (1 if R >= 5 else 0)
    n_plain = R - n_special
    na, nb = np.zeros(n_plain, np.int64), np.zeros(n_plain, np.int64)
    for r in range(n_plain):
        na[r], nb[r] = PAIRS[r] if r < len(PAIRS) else (rng.choice(LENGTHS), rng.choice(LENGTHS))
    if R >= 5:
        na, nb = np.append(na, 0), np.append(nb, 2)
    if R >= 3:
        na, nb = np.append(na, [64, 65]), np.append(nb, [63, 65])
    start_a, count_a, Pa = _layout(rng, na, gaps)
    start_b, count_b, Pb = _layout(rng, nb, gaps)
    if R >= 5:
        start_a[n_plain], count_a[n_plain] = -3, 10
    if R >= 1:
        Pa, Pb = Pa + 5, Pb + 3
        start_a, count_a = np.append(start_a, np.int32(Pa - 5)), np.append(count_a, np.int32(65))
        start_b, count_b = np.append(start_b, np.int32(Pb - 3)), np.append(count_b, np.int32(40))
    assert start_a.shape[0] == start_b.shape[0] == R
    case = {"R": R, "Pa": Pa, "Pb": Pb, "start_a": start_a, "count_a": count_a, "start_b": start_b, "count_b": count_b,
            "t_a": rng.random(Pa).astype(np.float32), "t_b": rng.random(Pb).astype(np.float32),  # (the rows of no ray: anything)
            "deltas_a": (0.5 + rng.random(Pa)).astype(np.float32), "deltas_b": (2.0 + rng.random(Pb)).astype(np.float32)}
    for r in range(R):
        (sa, ma), (sb, mb) = rows_of(case, "a", r), rows_of(case, "b", r)
        hi = (ma + mb) // 2 + 4
        ta, tb = np.sort(rng.integers(0, hi, ma)) / 64.0, np.sort(rng.integers(0, hi, mb)) / 64.0
        if R >= 3 and r == R - 2:
            tb = ta.copy()
        if R >= 3 and r == R - 3:
            ta = ta + tb.max() + 1.0 / 64.0
        for t in (ta, tb):
            t[(t == 0) & (rng.random(t.shape[0]) < 0.5)] = -0.0
        case["t_a"][sa:sa + ma], case["t_b"][sb:sb + mb] = ta, tb
    return case


def rows_of(case, which, r):
    s, n, P = int(case["start_" + which][r]), int(case["count_" + which][r]), case["P" + which]
    if s < 0 or s >= P or n <= 0:
        return 0, 0
    return s, min(n, P - s)


def empty_buffers(case, cap, pad=PAD):
    """the outputs of the write call, filled with sentinels: merged buffers of cap + pad rows, pos_a / pos_b, ray_count, total, overflow"""
    out = {k: np.full(cap + pad, SENTINEL_F, np.float32) for k in MERGED_F}
    out.update({k: np.full(cap + pad, SENTINEL_I, np.int32) for k in MERGED_I})
    out.update(pos_a=np.full(case["Pa"], SENTINEL_I, np.int32), pos_b=np.full(case["Pb"], SENTINEL_I, np.int32),
               ray_count=np.full(case["R"], SENTINEL_I, np.int32), total=np.full(1, SENTINEL_I, np.int32), overflow=np.full(1, 7, np.uint8))
    return out


def host_merge(lib, case, cap=None, pad=PAD):
    """The twin's two passes around numpy's exclusive sum.  cap None: the total.  -> dict with the fields of lab4d_amd.packed.MergedRays
    (numpy; the merged buffers have cap + pad rows, the last `pad` of which the twin must leave alone; total an int, overflow a bool) and
    `count`, the untruncated per-ray counts."""
    R = case["R"]
    count = np.full(R, SENTINEL_I, np.int32)
    p = lambda k: case[k].ctypes.data
    lib.pmerge_host_count(p("start_a"), p("count_a"), case["Pa"], p("start_b"), p("count_b"), case["Pb"], R, count.ctypes.data)
    incl = np.cumsum(count, dtype=np.int64)
    start = (incl - count).astype(np.int32)
    if cap is None:
        cap = int(incl[-1]) if R else 0
    out = empty_buffers(case, cap, pad)
    o = lambda k: out[k].ctypes.data
    lib.pmerge_host_write(p("t_a"), p("deltas_a"), p("start_a"), p("count_a"), case["Pa"], p("t_b"), p("deltas_b"), p("start_b"), p("count_b"), case["Pb"], R,
                          start.ctypes.data, cap, o("t"), o("deltas"), o("ray_idx"), o("src"), o("pos_a"), o("pos_b"), o("ray_count"), o("total"), o("overflow"))
    out.update(ray_start=start, total=int(out["total"][0]), overflow=bool(out["overflow"][0]), count=count, R=R, cap=cap)
    return out


def host_gather(lib, a, Pa, b, Pb, idx, C):
    """the twin's gather: a (Pa, C) / b (Pb, C) float32 or None, idx (n,) int32 -> out (n, C), pre-filled with the sentinel"""
    a = None if a is None else np.ascontiguousarray(a, np.float32)
    b = None if b is None else np.ascontiguousarray(b, np.float32)
    idx = np.ascontiguousarray(idx, np.int32)
    out = np.full((idx.shape[0], C), SENTINEL_F, np.float32)
    lib.pmerge_host_gather(None if a is None else a.ctypes.data, Pa, None if b is None else b.ctypes.data, Pb, idx.ctypes.data, idx.shape[0], C, out.ctypes.data)
    return out


def ref_merge(case, cap=None, pad=PAD):
    """The rules with numpy: per ray np.argsort(np.concatenate([t_a, t_b]), kind="stable") gives src, and from it everything else.  The
    same dict as host_merge, the rows behind the capacity at their sentinels."""
    R, Pa = case["R"], case["Pa"]
    rows = [(rows_of(case, "a", r), rows_of(case, "b", r)) for r in range(R)]
    count = np.array([ma + mb for (_, ma), (_, mb) in rows], np.int32).reshape(R)
    incl = np.cumsum(count, dtype=np.int64)
    start = (incl - count).astype(np.int32)
    total = int(incl[-1]) if R else 0
    if cap is None:
        cap = total
    out = empty_buffers(case, cap, pad)
    out["pos_a"][:], out["pos_b"][:] = -1, -1
    for r, ((sa, ma), (sb, mb)) in enumerate(rows):
        order = np.argsort(np.concatenate([case["t_a"][sa:sa + ma], case["t_b"][sb:sb + mb]]), kind="stable")
        from_b = order >= ma
        src = np.where(from_b, Pa + sb + order - ma, sa + order)
        t = np.where(from_b, case["t_b"][np.where(from_b, src - Pa, 0)], case["t_a"][np.where(from_b, 0, src)])
        deltas = np.where(from_b, case["deltas_b"][np.where(from_b, src - Pa, 0)], case["deltas_a"][np.where(from_b, 0, src)])
        dst = int(start[r]) + np.arange(ma + mb)
        live = dst < cap
        out["t"][dst[live]], out["deltas"][dst[live]], out["ray_idx"][dst[live]], out["src"][dst[live]] = t[live], deltas[live], r, src[live]
        out["pos_a"][src[live & ~from_b]] = dst[live & ~from_b]
        out["pos_b"][src[live & from_b] - Pa] = dst[live & from_b]
        out["ray_count"][r] = min(max(cap - int(start[r]), 0), ma + mb)
    first = min(total, cap)
    out["t"][first:cap], out["deltas"][first:cap], out["ray_idx"][first:cap], out["src"][first:cap] = 0, 0, -1, -1
    out.update(ray_start=start, total=total, overflow=total > cap, count=count, R=R, cap=cap)
    return out


def capacities(case, total, count, start):
    """total, total - 1, a cut in the middle of a ray (the longest ray's middle row), 0"""
    mid = int(start[int(np.argmax(count))]) + int(count.max()) // 2 if case["R"] else 0
    return sorted({total, max(total - 1, 0), mid, 0})


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, ref, what):
    """every output of the write call, the floats by their words, the rows behind the capacity included"""
    assert got["total"] == ref["total"] and got["overflow"] == ref["overflow"] and got["cap"] == ref["cap"], (what, got["total"], ref["total"])
    for k in ("count", "ray_start", "ray_count", "pos_a", "pos_b") + MERGED_I:
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (what, k)
    for k in MERGED_F:
        assert got[k].shape == ref[k].shape and np.array_equal(words(got[k]), words(ref[k])), (what, k, int((words(got[k]) != words(ref[k])).sum()))
