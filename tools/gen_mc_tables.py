#!/usr/bin/env python3
"""Generates lab4d_amd/csrc/mc_tables.hpp, the marching-cubes case table of csrc/mesh.hip and tests/host_harness/mesh_host.cpp.

The table is constructed, not transcribed (DESIGN.md "Iso-surface extraction"):
  * corner c of the cell at (i, j, k): bit 0 = +i, bit 1 = +j, bit 2 = +k (i is the slowest axis of the volume); bit c of the case
    index is set iff sdf[corner c] < level ("inside");
  * the 12 cell edges are the corner pairs that differ in one bit, numbered in ascending (a, b) order;
  * on each of the 6 cell faces the crossed edges are linked: 2 crossings -> one segment, 4 crossings (ambiguous face) -> two segments
    that cut off each INSIDE corner separately.  The rule reads only the face's four signs, so the two cells sharing a face agree;
  * every crossed edge then has degree 2: the segments form closed loops.  Each loop is oriented so that its normal points from the
    inside ends of its edges to the outside ends (towards increasing sdf) and triangulated as a fan whose diagonals do not lie in a
    cell face (the apex is rotated until none does): a diagonal inside an ambiguous face would coincide with the neighbour cell's
    segment there and give an edge with four triangles.

    python tools/gen_mc_tables.py            # rewrites the header in place
    python tools/gen_mc_tables.py --out F    # writes to F (the CPU test compares it byte for byte with the committed header)
"""
import argparse
import os

CORNER = [((c >> 0) & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]
EDGES = [(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1]
EDGE_ID = {e: n for n, e in enumerate(EDGES)}
MAX_TRIS = 5


def face_rings():
    """The 6 cell faces as corner rings in cyclic order."""
    rings = []
    for axis in range(3):
        for side in (0, 1):
            cs = [c for c in range(8) if ((c >> axis) & 1) == side]
            ring = [cs[0]]
            rest = cs[1:]
            while rest:
                nxt = [c for c in rest if bin(c ^ ring[-1]).count("1") == 1][0]
                ring.append(nxt)
                rest.remove(nxt)
            rings.append(ring)
    return rings


RINGS = face_rings()


def in_one_face(e0, e1):
    """Do the two cell edges lie in a common cell face?"""
    cs = set(EDGES[e0]) | set(EDGES[e1])
    return any(cs <= set(r) for r in RINGS)


def cross3(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def case_triangles(case):
    inside = [(case >> c) & 1 for c in range(8)]
    nbr = {}
    for ring in RINGS:
        edge = lambda n: EDGE_ID[tuple(sorted((ring[n % 4], ring[(n + 1) % 4])))]  # noqa: E731
        crossed = [n for n in range(4) if inside[ring[n]] != inside[ring[(n + 1) % 4]]]
        if len(crossed) == 2:
            segs = [(edge(crossed[0]), edge(crossed[1]))]
        elif len(crossed) == 4:
            segs = [(edge(n - 1), edge(n)) for n in range(4) if inside[ring[n]]]  # corner ring[n] sits between ring edges n-1 and n
        else:
            assert not crossed
            segs = []
        for a, b in segs:
            nbr.setdefault(a, []).append(b)
            nbr.setdefault(b, []).append(a)
    assert all(len(v) == 2 and v[0] != v[1] for v in nbr.values()), case
    assert sorted(nbr) == [n for n, (a, b) in enumerate(EDGES) if inside[a] != inside[b]], case
    tris, seen = [], set()
    for start in sorted(nbr):
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        while True:
            a, b = nbr[cur]
            nxt = a if a != prev else b
            if nxt == start:
                break
            loop.append(nxt)
            prev, cur = cur, nxt
        assert len(loop) >= 3 and len(set(loop)) == len(loop), (case, loop)
        seen.update(loop)
        # orientation: twice the loop's area vector (midpoints of the edges, doubled so that everything is an integer) against the
        # direction from the inside ends to the outside ends
        mid = [tuple(CORNER[EDGES[e][0]][d] + CORNER[EDGES[e][1]][d] for d in range(3)) for e in loop]
        area = [0, 0, 0]
        for n in range(len(loop)):
            c = cross3(mid[n], mid[(n + 1) % len(loop)])
            area = [area[d] + c[d] for d in range(3)]
        out_in = [0, 0, 0]
        for e in loop:
            a, b = EDGES[e]
            o, i = (b, a) if inside[a] else (a, b)
            out_in = [out_in[d] + CORNER[o][d] - CORNER[i][d] for d in range(3)]
        dot = sum(area[d] * out_in[d] for d in range(3))
        assert dot != 0, (case, loop)
        if dot < 0:
            loop = [loop[0]] + loop[:0:-1]
        fan = None
        for rot in range(len(loop)):
            cand = loop[rot:] + loop[:rot]
            if not any(in_one_face(cand[0], cand[n]) for n in range(2, len(cand) - 1)):
                fan = cand
                break
        assert fan is not None, (case, loop)
        tris += [(fan[0], fan[n], fan[n + 1]) for n in range(1, len(fan) - 1)]
    assert len(tris) <= MAX_TRIS, case
    return tris


def table():
    return [case_triangles(c) for c in range(256)]


def render():
    tab = table()
    lines = [
        "// Marching-cubes case table of csrc/mesh.hip and tests/host_harness/mesh_host.cpp.",
        "// GENERATED by tools/gen_mc_tables.py -- do not edit; tests/test_mesh_host.py regenerates it and compares byte for byte.",
        "// Corner c of the cell at (i, j, k): bit 0 = +i, bit 1 = +j, bit 2 = +k; case bit c set iff sdf[corner c] < level.",
        "// Edge e joins corners kEdgeCorner[e] and kEdgeCorner[e] + (1 << kEdgeAxis[e]): it is the +axis edge OWNED by that corner.",
        "// %d triangles in total, at most %d per case; kTriEdges[case] lists 3 edge numbers per triangle, 255 = unused." % (sum(len(t) for t in tab), MAX_TRIS),
        "#pragma once",
        "#include <stdint.h>",
        "",
        "namespace lab4d_mc {",
        "",
        "constexpr int kMaxTris = %d;" % MAX_TRIS,
        "constexpr uint8_t kEdgeCorner[12] = {%s};" % ", ".join(str(a) for a, _ in EDGES),
        "constexpr uint8_t kEdgeAxis[12] = {%s};" % ", ".join(str((a ^ b).bit_length() - 1) for a, b in EDGES),
        "constexpr uint8_t kTriCount[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tab[r:r + 32]) + ",")
    lines += ["};", "constexpr uint8_t kTriEdges[256][%d] = {" % (3 * MAX_TRIS)]
    for c, tris in enumerate(tab):
        flat = [e for t in tris for e in t]
        flat += [255] * (3 * MAX_TRIS - len(flat))
        lines.append("    {%s},  // %d" % (", ".join("%3d" % e for e in flat), c))
    lines += ["};", "", "}  // namespace lab4d_mc", ""]
    return "\n".join(lines)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(here), "lab4d_amd", "csrc", "mc_tables.hpp"))
    args = ap.parse_args()
    with open(args.out, "w") as fh:
        fh.write(render())


if __name__ == "__main__":
    main()
