"""Generates online_lang_splatting_amd/csrc/olsr_mc_table.h: the triangle table of the TSDF mesh extraction (k_tsdf.hip,
include/olsr.h "TSDF fusion", DESIGN.md "The mesh of the TSDF map").  The table is derived here from a rule, not typed in:

    python scripts/gen_mc_table.py            writes the header
    python scripts/gen_mc_table.py --check    exits 1 when the committed header differs from what this emits

Numbering.  Corner c of a cube sits at (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cube's lowest voxel; bit c of a
configuration is set when that corner's distance is negative.  Edge e = 4 * axis + k runs along `axis` (0 x, 1 y, 2 z) from
the corner whose two other coordinates, in ascending axis order, are (k & 1, k >> 1): it is the edge the voxel at that corner
owns along `axis`, so a table entry names a vertex of the surface extraction directly.

Rule, per configuration:
  - on each of the six faces the crossed face edges are joined by marching squares; a face with four crossings (the signs
    alternate round it) cuts each of its two NEGATIVE corners off by a segment of its own.  Only the face's four signs enter,
    so the two cubes that share a face draw the same segments on it;
  - every segment is directed so that, seen from outside the cube, the positive corners lie to its left.  Every crossed edge
    then ends one segment and starts another: the segments form closed directed loops over the crossed edges;
  - each loop is fanned from one of its edges, (e0, e_i, e_i+1), loops in the order of their lowest edge id.  The fan's apex
    e0 is the lowest edge id whose fan lays no diagonal into a face of the cube: a diagonal between two edges of one face
    (a face with four crossings, where the loop passes twice) would lie in that face, the neighbouring cube could lay the
    same one, and four triangles would share a side.  Fanning from the lowest id outright does that under every numbering of
    the edges (whichever edge is lowest, twelve loops through it get such a diagonal), and every loop has an apex that does
    not.  With the segments' direction cross(v_j - v_i, v_k - v_i) of a triangle (i, j, k) points to the positive
    (free-space) side.

No interior vertices and no asymptotic decider: ambiguous faces are always resolved the same way (DESIGN.md lists this among
the deviations from Lewiner's tables).  Packing: one 64-bit word per configuration, bits 0-3 the number of triangles (at most
5), then 4 bits per edge id, three per triangle.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "online_lang_splatting_amd", "csrc", "olsr_mc_table.h")
MAX_TRIANGLES = 5


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def corner_id(p):
    return int(p[0]) | int(p[1]) << 1 | int(p[2]) << 2


def edge_id(c0, c1):
    """The id of the edge between two neighbouring corners."""
    a, b = corner_offset(c0), corner_offset(c1)
    axis = [k for k in range(3) if a[k] != b[k]]
    assert len(axis) == 1
    others = [k for k in range(3) if k != axis[0]]
    return 4 * axis[0] + (a[others[0]] | a[others[1]] << 1)


def edge_corners(e):
    """(the corner the edge starts at — its owner —, the corner one step along its axis)."""
    axis, k = e >> 2, e & 3
    others = [d for d in range(3) if d != axis]
    p = [0, 0, 0]
    p[others[0]], p[others[1]] = k & 1, k >> 1
    q = list(p)
    q[axis] = 1
    return corner_id(p), corner_id(q)


def edge_midpoint(e):
    c0, c1 = edge_corners(e)
    return (np.array(corner_offset(c0), float) + np.array(corner_offset(c1), float)) / 2


def faces():
    """The six faces: (outward normal, its four corners in cyclic order)."""
    out = []
    for axis in range(3):
        u, v = [d for d in range(3) if d != axis]
        for side in (0, 1):
            normal = np.zeros(3)
            normal[axis] = 1.0 if side else -1.0
            ring = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[axis], p[u], p[v] = side, du, dv
                ring.append(corner_id(p))
            out.append((normal, ring))
    return out


FACES = faces()
FACE_EDGES = [{edge_id(ring[k], ring[(k + 1) % 4]) for k in range(4)} for _, ring in FACES]


def share_a_face(ea, eb):
    return any(ea in f and eb in f for f in FACE_EDGES)


def fan(loop):
    """The loop as triangles from the lowest apex whose diagonals all run through the cube's inside."""
    n = len(loop)
    for e0 in sorted(loop):
        r = loop[loop.index(e0):] + loop[:loop.index(e0)]
        if not any(share_a_face(r[0], r[k]) for k in range(2, n - 1)):
            return [(r[0], r[k], r[k + 1]) for k in range(1, n - 1)]
    raise AssertionError(loop)


def face_segments(config, face):
    """The directed marching-squares segments (edge id -> edge id) of one face under the rule above."""
    normal, ring = face
    neg = [(config >> c) & 1 for c in ring]
    crossed = [k for k in range(4) if neg[k] != neg[(k + 1) % 4]]      # face edge k joins ring[k] and ring[k + 1]
    if not crossed:
        return []
    if len(crossed) == 2:
        pairs = [(crossed[0], crossed[1], [k for k in range(4) if neg[k]][0])]
    else:   # the signs alternate: each negative corner is cut off by the two face edges that meet in it
        pairs = [((k - 1) % 4, k, k) for k in range(4) if neg[k]]
    out = []
    for ka, kb, kneg in pairs:
        ea, eb = edge_id(ring[ka], ring[(ka + 1) % 4]), edge_id(ring[kb], ring[(kb + 1) % 4])
        a, b = edge_midpoint(ea), edge_midpoint(eb)
        n = np.array(corner_offset(ring[kneg]), float)
        # seen from outside (the normal towards the eye) the negative corner must lie to the RIGHT of a -> b
        if np.dot(np.cross(normal, b - a), n - a) > 0:
            ea, eb = eb, ea
        out.append((ea, eb))
    return out


def triangles(config):
    """The triangles of one configuration as triples of edge ids."""
    succ = {}
    for face in FACES:
        for ea, eb in face_segments(config, face):
            assert ea not in succ, (config, ea)
            succ[ea] = eb
    assert sorted(succ) == sorted(succ.values()), config          # every crossed edge ends one segment and starts another
    tris, seen = [], set()
    for e0 in sorted(succ):
        if e0 in seen:
            continue
        loop, e = [e0], succ[e0]
        while e != e0:
            loop.append(e)
            e = succ[e]
        seen.update(loop)
        assert len(loop) >= 3
        tris += fan(loop)
    return tris


def table():
    """[256] lists of triangles."""
    t = [triangles(c) for c in range(256)]
    assert max(len(x) for x in t) <= MAX_TRIANGLES
    return t


def packed(t=None):
    """[256] ints: the 64-bit words of the header."""
    words = []
    for tris in (t or table()):
        w = len(tris)
        for k, e in enumerate(e for tri in tris for e in tri):
            w |= e << (4 + 4 * k)
        words.append(w)
    return words


def unpack(word):
    n = word & 15
    return [tuple((word >> (4 + 4 * (3 * k + j))) & 15 for j in range(3)) for k in range(n)]


def header_text():
    t = table()
    words = packed(t)
    lines = [
        "// olsr_mc_table.h — the triangle table of the TSDF mesh extraction (k_tsdf.hip).",
        "// GENERATED by scripts/gen_mc_table.py from the rule in its docstring; do not edit (tests/test_tsdf_mesh_cpu.py compares).",
        "// One word per sign configuration (bit c: corner c = (c & 1, c >> 1 & 1, c >> 2 & 1) is negative): bits 0-3 the number of",
        "// triangles, then 4 bits per edge id, three per triangle; edge 4 * axis + k is owned by the corner whose other two",
        f"// coordinates are (k & 1, k >> 1).  {sum(len(x) for x in t)} triangles in all, at most {max(len(x) for x in t)} per cube.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "namespace olsr {",
        "",
        "static __device__ const uint64_t MC_TABLE[256] = {",
    ]
    for r in range(0, 256, 4):
        lines.append("    " + " ".join(f"0x{w:016x}ull," for w in words[r:r + 4]))
    lines += ["};", "", "}  // namespace olsr", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    text = header_text()
    if a.check:
        sys.exit(0 if os.path.exists(HEADER) and open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    t = table()
    print(f"{HEADER}: {sum(len(x) for x in t)} triangles over 256 configurations, at most {max(len(x) for x in t)} per cube")
