"""Generates csrc/mc_tables.h, the marching-cubes case tables of the global-TSDF mesh extractor (csrc/tsdf_mesh.hip).

Nothing in the tables is typed by hand: for each of the 256 sign cases the crossing edges are joined into segments on
the six cube faces, the segments are chained into closed loops and every loop is fan-triangulated.

Conventions (shared with csrc/tsdf_mesh.hip and tests/mc_numpy.py):
* corner c = x + 2y + 4z sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cube's lowest corner; bit c of
  the case index is set when corner c is INSIDE (tsdf < level);
* edge e = 4 * axis + j runs from corner EDGE_CORNER[e] (its lower end) along `axis`; j enumerates the other two
  coordinate bits, so an edge is identified by the offset of its lower corner and its axis - the welding key;
* a face with four crossing edges (its inside corners diagonal) is resolved by one rule that reads only that face's
  four signs: the segments cut off the INSIDE corners.  Two cubes that share a face see the same signs, so they draw
  the same segments there and the mesh has no cracks;
* every segment is oriented so that, seen from outside the cube, the outside corners of the face lie to its left:
  the loops, and their fans, are then counter-clockwise seen from the free-space (positive tsdf) side.

Usage:  python tools/gen_mc_tables.py [--check]      (writes the header; --check only compares)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mast3r-slam-quality-dualtsdf_amd", "csrc", "mc_tables.h")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def _edges():
    """[(lower corner, axis)] for the 12 edges, e = 4 * axis + j."""
    out = []
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        for j in range(4):
            c = ((j & 1) << others[0]) | (((j >> 1) & 1) << others[1])
            out.append((c, axis))
    return out


EDGES = _edges()
EDGE_CORNER = [c for c, _ in EDGES]
EDGE_AXIS = [a for _, a in EDGES]


def edge_between(c0, c1):
    lo, hi = min(c0, c1), max(c0, c1)
    d = hi ^ lo
    assert d in (1, 2, 4)
    return EDGES.index((lo, d.bit_length() - 1))


def _faces():
    """[(outward normal, 4 corners in cyclic order)] for the 6 faces."""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            base = side << axis
            cyc = [base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)]
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            out.append((tuple(n), cyc))
    return out


FACES = _faces()


def _mid(e):
    p = list(corner_pos(EDGE_CORNER[e]))
    p[EDGE_AXIS[e]] += 0.5
    return p


def _sub(a, b):
    return [a[i] - b[i] for i in range(3)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return sum(a[i] * b[i] for i in range(3))


def face_segments(case, face):
    """Oriented segments (edge_from, edge_to) the face contributes, and whether the face was ambiguous."""
    n, cyc = face
    inside = [bool(case >> c & 1) for c in cyc]
    fedges = [edge_between(cyc[i], cyc[(i + 1) % 4]) for i in range(4)]     # fedges[i] joins cyc[i] and cyc[i+1]
    crossing = [inside[i] != inside[(i + 1) % 4] for i in range(4)]
    nx = sum(crossing)
    pairs = []   # (edge a, edge b, reference corner index into cyc or None)
    if nx == 2:
        i, j = [k for k in range(4) if crossing[k]]
        shared = None
        if j == i + 1:
            shared = j                  # fedges[i] and fedges[i+1] meet at cyc[i+1]
        elif i == 0 and j == 3:
            shared = 0                  # fedges[3] and fedges[0] meet at cyc[0]
        pairs.append((fedges[i], fedges[j], shared))
    elif nx == 4:
        # ambiguous face: cut off each inside corner (the two segments meet the two edges at that corner)
        for k in range(4):
            if inside[k]:
                pairs.append((fedges[(k - 1) % 4], fedges[k], k))
    segs = []
    for a, b, shared in pairs:
        # a segment between adjacent edges is oriented by the corner it cuts off; one between opposite edges splits the
        # face into two equal-sign halves, so any corner tells the side (edge midpoints never lie on a corner's line)
        ref = cyc[shared] if shared is not None else cyc[0]
        side = _dot(_cross(list(n), _sub(_mid(b), _mid(a))), _sub(list(corner_pos(ref)), _mid(a)))
        assert side != 0
        ref_inside = bool(case >> ref & 1)
        # outside corners to the left of a -> b (seen from outside): n x d points toward them
        if (side > 0) == ref_inside:
            a, b = b, a
        segs.append((a, b))
    return segs, nx == 4


def case_loops(case):
    nxt = {}
    for face in FACES:
        segs, _ = face_segments(case, face)
        for a, b in segs:
            assert a not in nxt, (case, a)
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        loops.append(loop)
    return loops


def build_tables():
    """-> (edge_table[256] 12-bit masks, tri_table[256] lists of (e0, e1, e2), tri_count[256])."""
    edge_table, tri_table = [], []
    for case in range(256):
        mask = 0
        for e, (c, axis) in enumerate(EDGES):
            if (case >> c & 1) != (case >> (c | (1 << axis)) & 1):
                mask |= 1 << e
        edge_table.append(mask)
        tris = []
        for loop in case_loops(case):
            for k in range(1, len(loop) - 1):
                tris.append((loop[0], loop[k], loop[k + 1]))
        tri_table.append(tris)
    return edge_table, tri_table, [len(t) for t in tri_table]


def render_header():
    edge_table, tri_table, tri_count = build_tables()
    max_tri = max(tri_count)
    out = ["// Generated by tools/gen_mc_tables.py - do not edit.  Marching-cubes case tables of csrc/tsdf_mesh.hip.",
           "// corner c = x + 2y + 4z; case bit c set = corner c inside (tsdf < level); edge e = 4 * axis + j runs from",
           "// kMcEdgeCorner[e] along kMcEdgeAxis[e].  Triangles are counter-clockwise seen from the positive-tsdf side.",
           "#pragma once",
           "#include <stdint.h>",
           "",
           "namespace mslam {",
           "",
           f"constexpr int kMcMaxTri = {max_tri};",
           "",
           "__constant__ const uint8_t kMcEdgeCorner[12] = {" + ", ".join(str(c) for c in EDGE_CORNER) + "};",
           "__constant__ const uint8_t kMcEdgeAxis[12] = {" + ", ".join(str(a) for a in EDGE_AXIS) + "};",
           "",
           "__constant__ const uint16_t kMcEdgeTable[256] = {"]
    for r in range(0, 256, 8):
        out.append("    " + ", ".join(f"0x{m:03x}" for m in edge_table[r:r + 8]) + ",")
    out += ["};", "", "__constant__ const uint8_t kMcTriCount[256] = {"]
    for r in range(0, 256, 16):
        out.append("    " + ", ".join(str(c) for c in tri_count[r:r + 16]) + ",")
    out += ["};", "", f"__constant__ const int8_t kMcTriTable[256][{3 * max_tri}] = {{"]
    for case in range(256):
        flat = [e for t in tri_table[case] for e in t]
        flat += [-1] * (3 * max_tri - len(flat))
        out.append("    {" + ", ".join(str(e) for e in flat) + "},")
    out += ["};", "", "}  // namespace mslam", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true", help="exit 1 when the committed header differs")
    args = ap.parse_args()
    text = render_header()
    if args.check:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("mc_tables.h is up to date" if same else "mc_tables.h differs from the generator's output")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(f"wrote {HEADER}")


if __name__ == "__main__":
    main()
