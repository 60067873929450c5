"""numpy restatement of the TSDF volume's triangle mesh (include/regnet_hip.h "Triangle mesh", DESIGN.md par. 5), written from
the contract text and not from csrc/tsdf_mesh.hip or csrc/tsdf_mesh_table.h: the generator of the 256-case table, the mesh of a
``tsdf_reference.Volume`` as plain loops over its cells, and the vertex rows looked up by key in that volume's extraction.  Not
a test.

The table's rule.  Corner ``c`` of a cell is its low corner voxel plus ``(c & 1, c >> 1 & 1, c >> 2 & 1)``; a corner is INSIDE
when ``D < 0``; a case is the 8-bit mask of inside corners.  Edge ``(c, a)`` joins corner ``c`` (bit ``a`` clear) to corner
``c | 1 << a``; the twelve edges are numbered in ascending ``(c, a)``; an edge is CROSSED when one end is inside.

1. Faces.  Face ``(k, s)`` holds the four corners whose bit ``k`` is ``s``.  With ``u = (k + 1) % 3`` and ``v = (k + 2) % 3`` they
   are taken in the cyclic order ``q0..q3 = (0,0), (1,0), (1,1), (0,1)`` of their ``(u, v)`` bits -- counterclockwise seen from
   ``+e_k`` --, and face edge ``E_i`` joins ``q_i`` to ``q_(i+1)``.  Every maximal run ``q_i .. q_j`` of inside corners in that
   cyclic order (not none, not all four) gives ONE segment, which cuts that run off: it joins ``E_(i-1)`` to ``E_j``.  Two
   diagonal inside corners are two runs of one, so each is cut off by its own segment, and the choice depends on the face's four
   signs only: two cells that share a face agree on it.
2. Direction.  Seen from outside the cell the segment runs CLOCKWISE round the corners it cuts off (they are on its right,
   ``D > 0`` on its left): from ``E_(i-1)`` to ``E_j`` on a face ``s = 1``, from ``E_j`` to ``E_(i-1)`` on a face ``s = 0``.  A
   surface patch whose boundary runs that way has its right-hand-rule normal towards ``D > 0``.
3. Loops.  Every crossed edge lies in two faces, ends one segment and starts one: the segments chain into closed directed loops
   of 3 to 7 edges.  The loops of a case are taken in ascending order of their lowest edge.
4. Fan.  A loop ``v_0 .. v_(n-1)`` from its APEX ``v_0`` becomes the triangles ``(v_0, v_i, v_(i+1))``, ``i = 1 .. n - 2``.  A fan
   diagonal ``(v_0, v_i)``, ``1 < i < n - 1``, whose two edges lie in one cube face is FLAT: it runs inside that face, where the
   neighbouring cell has no matching side.  The apex is the edge of the loop with the fewest flat diagonals, the lowest edge
   number among equals.
"""
import numpy as np

from . import tsdf_reference as ref

CORNERS = tuple((c & 1, c >> 1 & 1, c >> 2 & 1) for c in range(8))
EDGES = tuple((c, a) for c in range(8) for a in range(3) if not c >> a & 1)      # edge number -> (corner, axis)
EDGE_ID = {ca: e for e, ca in enumerate(EDGES)}
FACES = tuple((k, s) for k in range(3) for s in range(2))
MAX_TRIANGLES_PER_CASE = 5


def edge_ends(e):
    """-> the two corners of edge ``e``."""
    c, a = EDGES[e]
    return c, c | 1 << a


def edge_between(c0, c1):
    """The edge that joins two corners which differ in one bit."""
    lo = min(c0, c1)
    return EDGE_ID[(lo, (c0 ^ c1).bit_length() - 1)]


def face_corners(k, s):
    """The corners q0..q3 of face ``(k, s)`` in the rule's cyclic order."""
    u, v = (k + 1) % 3, (k + 2) % 3
    return [s << k | qu << u | qv << v for qu, qv in ((0, 0), (1, 0), (1, 1), (0, 1))]


def face_edges(k, s):
    """-> E_0..E_3 of face ``(k, s)``: ``E_i`` joins ``q_i`` and ``q_(i+1)``."""
    q = face_corners(k, s)
    return [edge_between(q[i], q[(i + 1) % 4]) for i in range(4)]


def same_face(e0, e1):
    """Whether two edges lie in one cube face."""
    (c0, a0), (c1, a1) = EDGES[e0], EDGES[e1]
    return any(k != a0 and k != a1 and (c0 >> k & 1) == (c1 >> k & 1) for k in range(3))


def face_segments(case, k, s):
    """The directed segments ``(from edge, to edge)`` of face ``(k, s)`` under ``case``: steps 1 and 2 of the rule."""
    q, E = face_corners(k, s), face_edges(k, s)
    inside = [case >> c & 1 for c in q]
    if sum(inside) in (0, 4):
        return []
    out = []
    for i in range(4):
        if inside[i] and not inside[(i - 1) % 4]:          # a run starts at q_i
            j = i
            while inside[(j + 1) % 4]:
                j = (j + 1) % 4
            first, last = E[(i - 1) % 4], E[j]
            out.append((first, last) if s == 1 else (last, first))
    return out


def crossed_edges(case):
    return [e for e in range(12) if (case >> edge_ends(e)[0] & 1) != (case >> edge_ends(e)[1] & 1)]


def case_loops(case, prefer_unflat_apex=True):
    """The directed loops of ``case``, each rotated to start at its apex: steps 3 and 4."""
    nxt = {}
    for k, s in FACES:
        for a, b in face_segments(case, k, s):
            assert a not in nxt
            nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values()) == crossed_edges(case)
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        n = len(loop)
        assert 3 <= n <= 7
        best = 0                                            # (the loop starts at its lowest edge)
        if prefer_unflat_apex:
            def flat(j):
                return sum(same_face(loop[j], loop[(j + i) % n]) for i in range(2, n - 1))
            best = min(range(n), key=lambda j: (flat(j), loop[j]))
        loops.append(loop[best:] + loop[:best])
    return loops


def flat_diagonals(loop):
    n = len(loop)
    return sum(same_face(loop[0], loop[i]) for i in range(2, n - 1))


def case_triangles(case, prefer_unflat_apex=True):
    """-> the triangles of ``case`` as triples of edge numbers, in the table's order."""
    out = []
    for loop in case_loops(case, prefer_unflat_apex):
        out += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    assert len(out) <= MAX_TRIANGLES_PER_CASE
    return out


def make_table(prefer_unflat_apex=True):
    """-> (256, 16) int8: row ``case`` holds its triangles' edge numbers, three per triangle, -1 in the unused slots."""
    table = np.full((256, 16), -1, dtype=np.int8)
    for case in range(256):
        flat = [e for tri in case_triangles(case, prefer_unflat_apex) for e in tri]
        table[case, :len(flat)] = flat
    return table


TABLE = make_table()
TRIANGLES = (TABLE >= 0).sum(axis=1) // 3


def usable(vol, min_weight=None):
    """Per voxel ``W >= min_weight && D < 1`` (a NaN is not) -> (N) bool."""
    mw = np.int32(vol.p["min_weight"] if min_weight is None else min_weight)
    with np.errstate(invalid="ignore"):
        return (vol.W >= mw) & (vol.D < np.float32(1.0))


def cells(vol):
    """Plain loops over the cells of ``vol`` in ascending ``l`` -> [(l, case)] of the MESHED cells whose case has triangles."""
    nx, ny, nz = vol.dims
    ok = usable(vol)
    with np.errstate(invalid="ignore"):
        inside = vol.D < np.float32(0.0)
    out = []
    for iz in range(nz - 1):
        for iy in range(ny - 1):
            for ix in range(nx - 1):
                l = (iz * ny + iy) * nx + ix
                if not ok[l]:
                    continue
                corners = [l + dx + dy * nx + dz * nx * ny for dx, dy, dz in CORNERS]
                if not all(ok[v] for v in corners):
                    continue
                case = sum(int(inside[v]) << c for c, v in enumerate(corners))
                if TRIANGLES[case]:
                    out.append((l, case))
    return out


def mesh(vol, max_triangles, extraction=None):
    """The mesh of ``vol`` (a ``tsdf_reference.Volume``, whose ``min_weight`` and ``max_points`` hold) -> dict(``tri``
    (max_triangles,3) int32, ``num`` (4) int32 = (Kt, Tt, dropped, overflow), ``cells`` (Tt) int64: the cell of every triangle,
    ``surface``: ``vol.extract()``'s dict).  The vertex of edge ``(c, a)`` of cell ``l`` is the row whose key is ``3 l(voxel of
    c) + a``; a triangle with a vertex row at or beyond the surface's K is written as (-1, -1, -1) in its place."""
    nx, ny, _ = vol.dims
    surface = vol.extract() if extraction is None else extraction
    row_of = {int(key): row for row, key in enumerate(surface["keys"])}       # (the K kept rows only)
    mt = int(max_triangles)
    tri = np.full((mt, 3), -1, dtype=np.int32)
    total = dropped = 0
    owner = []
    for l, case in cells(vol):
        for t in range(TRIANGLES[case]):
            if total < mt:
                rows = []
                for e in TABLE[case, 3 * t:3 * t + 3]:
                    c, a = EDGES[e]
                    dx, dy, dz = CORNERS[c]
                    rows.append(row_of.get(3 * (l + dx + dy * nx + dz * nx * ny) + a, -1))
                if min(rows) < 0:
                    dropped += 1
                else:
                    tri[total] = rows
            owner.append(l)
            total += 1
    num = np.array([min(total, mt), total, dropped, 1 if total > mt else 0], dtype=np.int32)
    return {"tri": tri, "num": num, "cells": np.array(owner, dtype=np.int64), "surface": surface}


def sign_field_mesh(inside):
    """The mesh of a bare sign field ``inside`` [iz, iy, ix] bool, every corner usable, with one vertex per crossed voxel edge
    named by its key -> (T,3) int64 of keys.  For the topology tests, which need no distances."""
    nz, ny, nx = inside.shape
    flat = inside.reshape(-1)
    out = []
    for iz in range(nz - 1):
        for iy in range(ny - 1):
            for ix in range(nx - 1):
                l = (iz * ny + iy) * nx + ix
                corners = [l + dx + dy * nx + dz * nx * ny for dx, dy, dz in CORNERS]
                case = sum(int(flat[v]) << c for c, v in enumerate(corners))
                for t in range(TRIANGLES[case]):
                    out.append([3 * corners[EDGES[e][0]] + EDGES[e][1] for e in TABLE[case, 3 * t:3 * t + 3]])
    return np.array(out, dtype=np.int64).reshape(-1, 3)
