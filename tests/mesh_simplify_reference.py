"""Plain-loop restatement of the mesh simplification (include/regnet_hip.h "Mesh simplification", DESIGN.md par. 5), written from
the contract text and not from csrc/mesh_simplify.hip: float32 for the cell arithmetic (numpy rounds every operation on its own;
its division is correctly rounded), Python ints for the sums, a ``dict`` for the triangle set, float64 for the finalise.  Not a
test.
"""
import math

import numpy as np

f32 = np.float32
f64 = np.float64
QNAN = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def grid_for(dims, voxel, cell):
    """``Mesh.simplify``'s grid: ``g_k = ceil(n_k voxel / cell) + 1``, in float64."""
    return tuple(int(math.ceil(int(n) * float(voxel) / float(cell))) + 1 for n in dims)


def vertex_cell(p, origin, cell_f, grid):
    """One vertex (3 float32) -> (cell, (ix, iy, iz), (fx, fy, fz) float32), or (-1, None, None) for a STRAY one."""
    i, f = [], []
    for k in range(3):
        x = f32(p[k])
        if not np.isfinite(x):
            return -1, None, None
        with np.errstate(all="ignore"):
            d = f32(x - f32(origin[k]))
            a = f32(d / cell_f)
            fl = np.floor(a)
        assert isinstance(a, np.float32) and isinstance(fl, np.float32)
        if not (fl >= f32(0.0) and fl < f32(grid[k])):       # (a NaN or infinite quotient fails)
            return -1, None, None
        ik = int(fl)
        i.append(ik)
        f.append(f32(a - f32(ik)))
    return (i[2] * grid[1] + i[1]) * grid[0] + i[0], tuple(i), tuple(f)


def _colour(c):
    c = f32(c)
    if not c > f32(0.0):                                      # (a NaN too)
        return 0
    return int(np.rint(f32(min(c, f32(1.0)) * f32(255.0))))


def _normal(n):
    n = f32(n)
    return int(np.rint(f32(min(max(n, f32(-1.0)), f32(1.0)) * f32(1048576.0))))


def simplify(xyz, normal, rgb, K, tri, Kt, origin, cell, grid, dedupe, max_vertices, max_triangles):
    """-> dict(``xyz`` / ``normal`` / ``rgb`` (max_vertices,3) float32, ``weight`` (max_vertices) int32, ``tri`` (max_triangles,3)
    int32, ``num`` (12) int32, ``surface_num`` (4) int32, and for the tests ``cells`` (Kv) int64: the cell of every new vertex in
    all, ``vertex_cell`` (K) int64: the cell of every source vertex (-1: STRAY), ``source`` (survivors) int64: the source row of
    every survivor in all)."""
    xyz, normal, rgb = (np.asarray(a, dtype=np.float32).reshape(-1, 3) for a in (xyz, normal, rgb))
    tri = np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    K, Kt = int(K), int(Kt)
    gx, gy, gz = (int(g) for g in grid)
    origin = np.asarray(origin, dtype=np.float32)
    cell_f = f32(float(cell))
    mv, mt = int(max_vertices), int(max_triangles)
    # ---- vertices into cells: integers only ------------------------------------------------------------------------------
    cells = {}
    of_vertex = np.full((K,), -1, dtype=np.int64)
    stray_vertices = 0
    for r in range(K):
        c, _, f = vertex_cell(xyz[r], origin, cell_f, grid)
        if c < 0:
            stray_vertices += 1
            continue
        of_vertex[r] = c
        acc = cells.setdefault(c, dict(count=0, S=[0, 0, 0], C=[0, 0, 0], N=[0, 0, 0], ncount=0, first=r))
        acc["count"] += 1
        acc["first"] = min(acc["first"], r)
        for k in range(3):
            acc["S"][k] += int(f32(f[k] * f32(16777216.0)))   # (truncated; the product is below 2^24)
            acc["C"][k] += _colour(rgb[r, k])
        if np.isfinite(normal[r]).all():
            for k in range(3):
                acc["N"][k] += _normal(normal[r, k])
            acc["ncount"] += 1
    # ---- triangles ------------------------------------------------------------------------------------------------------
    stray = collapsed = duplicate = 0
    keys = []                                                   # (source row, (c0, c1, c2)) of the rows that may survive
    for t in range(Kt):
        v = [int(x) for x in tri[t]]
        if v == [-1, -1, -1] or any(not 0 <= x < K for x in v) or any(of_vertex[x] < 0 for x in v):
            stray += 1                                          # ABSENT and STRAY share a counter
            continue
        c = [int(of_vertex[x]) for x in v]
        if c[0] == c[1] or c[1] == c[2] or c[2] == c[0]:
            collapsed += 1
            continue
        lo = c.index(min(c))
        keys.append((t, (c[lo], c[(lo + 1) % 3], c[(lo + 2) % 3])))
    if dedupe:
        smallest = {}
        for t, key in keys:
            smallest[key] = min(smallest.get(key, t), t)
        survivors = [(t, key) for t, key in keys if smallest[key] == t]
        duplicate = len(keys) - len(survivors)
    else:
        survivors = keys
    # ---- outputs --------------------------------------------------------------------------------------------------------
    used = sorted({c for _, key in survivors for c in key})
    new_row = {c: row for row, c in enumerate(used)}
    kv_all, kv = len(used), min(len(used), mv)
    out_xyz = np.full((mv, 3), QNAN, dtype=np.float32)
    out_normal = np.full((mv, 3), QNAN, dtype=np.float32)
    out_rgb = np.zeros((mv, 3), dtype=np.float32)
    out_weight = np.full((mv,), -1, dtype=np.int32)
    for row, c in enumerate(used[:kv]):
        acc = cells[c]
        n = acc["count"]
        out_weight[row] = n
        if n == 1:
            out_xyz[row], out_normal[row], out_rgb[row] = xyz[acc["first"]], normal[acc["first"]], rgb[acc["first"]]
            continue
        i = (c % gx, c // gx % gy, c // gx // gy)
        m = []
        for k in range(3):
            q = f64(acc["S"][k]) / (f64(n) * f64(16777216.0))
            a = f64(i[k]) + q
            b = a * f64(cell_f)
            out_xyz[row, k] = f32(f64(origin[k]) + b)
            out_rgb[row, k] = f32(f64(acc["C"][k]) / (f64(n) * f64(255.0)))
            m.append(f64(acc["N"][k]) / f64(1048576.0))
        length = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
        if acc["ncount"] != 0 and length != 0.0:
            for k in range(3):
                out_normal[row, k] = f32(m[k] / length)
    out_tri = np.full((mt, 3), -1, dtype=np.int32)
    dropped = 0
    for row, (_, key) in enumerate(survivors[:mt]):
        rows = [new_row[c] for c in key]
        if max(rows) >= mv:
            dropped += 1
        else:
            out_tri[row] = rows
    num = np.array([kv, kv_all, kv_all > mv, len(cells), stray_vertices, min(len(survivors), mt), len(survivors), dropped,
                    len(survivors) > mt, collapsed, duplicate, stray], dtype=np.int32)
    return {"xyz": out_xyz, "normal": out_normal, "rgb": out_rgb, "weight": out_weight, "tri": out_tri, "num": num,
            "surface_num": np.array([kv, kv_all, K, kv_all > mv], dtype=np.int32),
            "cells": np.array(used, dtype=np.int64), "vertex_cell": of_vertex,
            "source": np.array([t for t, _ in survivors], dtype=np.int64)}


def directed_edges(tri):
    """-> Counter of the directed edges of (M,3) triangles."""
    import collections
    use = collections.Counter()
    for a, b, c in np.asarray(tri).tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            use[(x, y)] += 1
    return use


def balanced(tri):
    """Every directed edge (a, b) occurs as often as (b, a)."""
    use = directed_edges(tri)
    return all(use[(y, x)] == n for (x, y), n in use.items())
