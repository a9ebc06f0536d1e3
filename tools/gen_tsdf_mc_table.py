"""The marching-cubes case table of tdv_tsdf_extract_mesh_dev, made from rule T11 of include/tdv_hip.h (no hand-made table is copied).

    python tools/gen_tsdf_mc_table.py            writes 3dvision_amd/csrc/tsdf_mc_table.hpp
    python tools/gen_tsdf_mc_table.py --check    exits 1 unless the committed header equals what the rule gives

Corner q of the unit cube is (q & 1, (q >> 1) & 1, (q >> 2) & 1) (T9); edge e = 4*axis + idx starts at its owner corner (T10).  A case is
the set of negative corners.  table() returns, per case, the list of triangles as triples of edge numbers; packed() the committed form,
256 rows of 16 bytes: the triangle count, then 15 edge numbers (FILL where a row has fewer).  Pure Python: tests/tsdf_mesh_restatement.py
and tests/test_tsdf_mesh_abi.py import it."""
import os
import sys

FILL = 255
MAX_TRIANGLES = 5
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "3dvision_amd", "csrc", "tsdf_mc_table.hpp")


def corner(q):
    return (q & 1, (q >> 1) & 1, (q >> 2) & 1)


def corner_number(c):
    return c[0] + 2 * c[1] + 4 * c[2]


def edge_owner(e):
    """T10: the corner at which edge e starts."""
    axis, idx = e >> 2, e & 3
    a, b = idx & 1, idx >> 1
    return ((0, a, b), (a, 0, b), (a, b, 0))[axis]


def edge_ends(e):
    """(owner corner number, the other end's)."""
    o = list(edge_owner(e))
    far = list(o)
    far[e >> 2] = 1
    return corner_number(o), corner_number(far)


def edge_mid(e):
    """Twice the midpoint of edge e (integers)."""
    a, b = (corner(q) for q in edge_ends(e))
    return tuple(a[d] + b[d] for d in range(3))


def face_edges(axis, side):
    """The four edges of the face `axis` = side."""
    return [e for e in range(12) if all(corner(q)[axis] == side for q in edge_ends(e))]


FACES = [(axis, side) for axis in range(3) for side in (0, 1)]


def on_common_face(e0, e1):
    return any(e0 in face_edges(*f) and e1 in face_edges(*f) for f in FACES)


def crossing(case, e):
    a, b = edge_ends(e)
    return ((case >> a) & 1) != ((case >> b) & 1)


def segments(case):
    """T11.1: the face segments of a case, as unordered pairs of edges."""
    out = []
    for f in FACES:
        es = [e for e in face_edges(*f) if crossing(case, e)]
        assert len(es) in (0, 2, 4)
        if len(es) == 2:
            out.append((es[0], es[1]))
        elif len(es) == 4:
            # the negative corners lie on a diagonal: each is cut off by the two face edges that meet at it
            neg = [q for q in range(8) if corner(q)[f[0]] == f[1] and (case >> q) & 1]
            assert len(neg) == 2
            for q in neg:
                pair = [e for e in es if q in edge_ends(e)]
                assert len(pair) == 2
                out.append((pair[0], pair[1]))
    return out


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def loops(case):
    """T11.2 to T11.4: the closed loops of a case, each from its smallest edge in the direction T11.3 fixes, in ascending smallest edge."""
    nb = {}
    for a, b in segments(case):
        nb.setdefault(a, []).append(b)
        nb.setdefault(b, []).append(a)
    assert all(len(v) == 2 and v[0] != v[1] for v in nb.values())                  # two segments, to two different edges
    assert sorted(nb) == [e for e in range(12) if crossing(case, e)]
    out, seen = [], set()
    for start in sorted(nb):
        if start in seen:
            continue
        loop, prev, cur = [start], start, nb[start][0]
        while cur != start:
            loop.append(cur)
            prev, cur = cur, (nb[cur][1] if nb[cur][0] == prev else nb[cur][0])
        assert len(loop) >= 3 and len(set(loop)) == len(loop)
        seen.update(loop)
        N = [0, 0, 0]
        for i in range(len(loop)):
            c = _cross(edge_mid(loop[i]), edge_mid(loop[(i + 1) % len(loop)]))
            N = [N[d] + c[d] for d in range(3)]
        D = [0, 0, 0]
        for e in loop:
            a, b = edge_ends(e)
            neg, pos = (a, b) if (case >> a) & 1 else (b, a)
            D = [D[d] + corner(pos)[d] - corner(neg)[d] for d in range(3)]
        dot = sum(N[d] * D[d] for d in range(3))
        assert dot != 0, (case, loop)
        if dot < 0:
            loop = [loop[0]] + loop[:0:-1]
        out.append(loop)
    return out


def fan_start(loop):
    """T11.5: the first rotation whose fan diagonals all leave the cube's faces."""
    n = len(loop)
    for r in range(n):
        rot = loop[r:] + loop[:r]
        if not any(on_common_face(rot[0], rot[i]) for i in range(2, n - 1)):
            return r
    raise AssertionError("no rotation keeps the fan's diagonals off the faces: %r" % (loop,))


def triangles(case):
    out = []
    for loop in loops(case):
        r = fan_start(loop)
        rot = loop[r:] + loop[:r]
        out += [(rot[0], rot[i], rot[i + 1]) for i in range(1, len(rot) - 1)]
    return out


_TABLE = []


def table():
    """[256] lists of (e0, e1, e2)."""
    if not _TABLE:
        _TABLE.extend(triangles(case) for case in range(256))
        assert max(len(t) for t in _TABLE) == MAX_TRIANGLES
    return _TABLE


def packed():
    """bytes, 256 x 16: count, 15 edge numbers."""
    out = bytearray()
    for tris in table():
        row = [len(tris)] + [e for t in tris for e in t]
        out += bytes(row + [FILL] * (16 - len(row)))
    assert len(out) == 4096
    return bytes(out)


def stats():
    """The figures the rule's statement lists."""
    t = table()
    counts = [len(x) for x in t]
    shifts = [fan_start(loop) for case in range(256) for loop in loops(case)]
    return dict(triangles=sum(counts), most=max(counts), histogram=[counts.count(k) for k in range(max(counts) + 1)],
                rotated=[shifts.count(k) for k in range(1, max(shifts) + 1)])


def header_text():
    p = packed()
    lines = ["// Generated by tools/gen_tsdf_mc_table.py from rule T11 of include/tdv_hip.h; do not edit.  tests/test_tsdf_mesh_abi.py holds it to the generator.",
             "// 256 cases x 16 bytes: the triangle count, then 15 cell edge numbers (T10), 255 where the case has fewer triangles.",
             "#pragma once",
             "alignas(16) static __device__ const unsigned char TS_MC_TABLE[256 * 16] = {"]
    for case in range(256):
        lines.append("    " + ",".join("%3d" % b for b in p[16 * case:16 * case + 16]) + ("," if case < 255 else " ") + "  // %3d" % case)
    lines.append("};")
    return "\n".join(lines) + "\n"


def parse_header(text):
    """The bytes of a header header_text() wrote."""
    body = text.split("TS_MC_TABLE[256 * 16] = {", 1)[1].rsplit("};", 1)[0]
    vals = []
    for line in body.split("\n"):
        line = line.split("//")[0].strip()
        vals += [int(v) for v in line.split(",") if v.strip()]
    return bytes(vals)


if __name__ == "__main__":
    if "--check" in sys.argv[1:]:
        ok = open(HEADER).read() == header_text()
        print("tsdf_mc_table.hpp %s the generator" % ("equals" if ok else "DIFFERS FROM"))
        sys.exit(0 if ok else 1)
    with open(HEADER, "w") as fh:
        fh.write(header_text())
    print(stats())
