"""tests/mesh_simplify_reference.py -- the plain-loop restatement of the mesh simplification -- held to things it can be wrong
about, on two closed meshes: a sphere and a box, each rendered from 26 directions, fused by tests/tsdf_reference.py at 24^3 and
meshed by tests/tsdf_mesh_reference.py.  No GPU: the library is loaded for the host-only accessors alone.

The bound ``E``.  A vertex coordinate x goes through d = fl(x - o) and a = fl(d / c): a = (x - o) / c (1 + e1)(1 + e2) with |e| <=
2^-24, so i = floor(a) places x - o within eta = (i + 1) c (2^-23 + 2^-48) <= 2^-22 * (g c) of [i c, (i + 1) c].  The image of a cell
is a mean of points o + (i + f) c, 0 <= f < 1, inside that interval in exact arithmetic; its float64 evaluation is off by parts
in 2^50 and the one rounding to float32 by at most 2^-24 |x|.  A cell with one vertex keeps it: distance 0.  Per axis therefore
|x - image| <= c + tol with tol = 2^-22 (g c) + 2^-23 max|x| (the second term doubled to cover the float64 parts), and E = sqrt(3)
tol.  Nothing here is taken from what the code gives.
"""
import itertools

import numpy as np
import pytest

from . import mesh_simplify_reference as sref
from . import tsdf_mesh_reference as mref
from . import tsdf_reference as ref
from .icp_projective_reference import look_at, rectangle, render, sphere

f32 = np.float32
W, H = 64, 48
K = (150.0, 150.0, 31.5, 23.5)
CENTRE = np.array([0.011, -0.007, 0.503])


def views(centre, distance=0.3):
    """26 cameras round ``centre``: along every axis, face diagonal and space diagonal."""
    out = []
    for d in itertools.product((-1, 0, 1), repeat=3):
        if d == (0, 0, 0):
            continue
        d = np.array(d, dtype=np.float64)
        d /= np.linalg.norm(d)
        up = (0.0, 0.0, 1.0) if abs(d[2]) < 0.9 else (0.0, 1.0, 0.0)
        out.append(look_at(centre + distance * d, centre, up=up))
    return out


def box(centre, half):
    """The six faces of an axis-aligned box as ``rectangle``s."""
    c, h = np.asarray(centre, dtype=np.float64), np.asarray(half, dtype=np.float64)
    out = []
    for k in range(3):
        u, v = (k + 1) % 3, (k + 2) % 3
        for side in (-1, 1):
            o = c - h
            o[k] = c[k] + side * h[k]
            a, b = np.zeros(3), np.zeros(3)
            a[u], b[v] = 2 * h[u], 2 * h[v]
            out.append(rectangle(o, a, b))
    return out


def scene_params(n, voxel=0.004):
    return dict(voxel=voxel, trunc=5 * voxel, origin=tuple(CENTRE - n * voxel / 2), dims=(n, n, n), max_points=1 << 14)


def scene_views(kind, scale=1.0):
    """-> (clouds, shapes, poses) of the 26 rendered views of the sphere or the box."""
    if kind == "sphere":
        scene = [sphere(CENTRE, 0.029 * scale)]
    else:
        scene = box(CENTRE + np.array([0.001, 0.002, -0.001]), np.array([0.027, 0.021, 0.03]) * scale)
    poses = views(CENTRE)
    clouds = [(render(scene, W, H, K, pose), None) for pose in poses]
    return clouds, [(W, H, K)] * len(poses), poses


_SCENES = {}


def fused(kind):
    """-> (the ``tsdf_reference.Volume``, ``tsdf_mesh_reference.mesh``'s dict) of a scene at 24^3; computed once, not changed."""
    if kind not in _SCENES:
        vol, _, surface = ref.fuse_volume(*scene_views(kind), **scene_params(24))
        _SCENES[kind] = (vol, mref.mesh(vol, 1 << 15, surface))
    return _SCENES[kind]


def run(kind, factor, dedupe, max_vertices=1 << 14, max_triangles=1 << 15):
    vol, mesh = fused(kind)
    s = mesh["surface"]
    cell = factor * float(vol.p["voxel"])
    grid = sref.grid_for(vol.dims, vol.p["voxel"], cell)
    out = sref.simplify(s["xyz"], s["normal"], s["rgb"], s["num"][0], mesh["tri"], mesh["num"][0], vol.origin, cell, grid, dedupe,
                        max_vertices, max_triangles)
    return vol, mesh, out, cell, grid


def tolerance(vol, cell, grid, xyz):
    extent = max(grid) * float(f32(cell))
    return 2.0 ** -22 * extent + 2.0 ** -23 * float(np.abs(xyz).max())


@pytest.mark.parametrize("kind", ["sphere", "box"])
def test_the_source_scene_is_closed_and_has_no_stray_vertex(kind):
    vol, mesh = fused(kind)
    kt = int(mesh["num"][0])
    assert kt > 2000 and mesh["num"].tolist() == [kt, kt, 0, 0]
    use = sref.directed_edges(mesh["tri"][:kt])
    assert all(n == 1 for n in use.values()) and all((y, x) in use for x, y in use)      # no hole
    _, _, out, _, _ = run(kind, 4, 1)
    assert out["num"][4] == 0 and out["num"][11] == 0 and (out["vertex_cell"] >= 0).all()


@pytest.mark.parametrize("kind", ["sphere", "box"])
@pytest.mark.parametrize("factor", [2, 4])
def test_new_vertices_lie_in_their_cells_and_near_their_sources(kind, factor):
    vol, mesh, out, cell, grid = run(kind, factor, 1)
    kv = int(out["num"][0])
    assert kv == out["num"][1] == len(out["cells"]) > 10
    cells = out["cells"]
    index = np.stack([cells % grid[0], cells // grid[0] % grid[1], cells // grid[0] // grid[1]], axis=1).astype(np.float64)
    c, o = float(f32(cell)), vol.origin.astype(np.float64)
    got = out["xyz"][:kv].astype(np.float64)
    source = mesh["surface"]["xyz"][:int(mesh["surface"]["num"][0])].astype(np.float64)
    tol = tolerance(vol, cell, grid, source)
    assert (got >= o + index * c - tol).all() and (got <= o + (index + 1) * c + tol).all()
    # every source vertex whose cell was emitted is within sqrt(3) cell + E of its image
    row_of = {int(cell_): row for row, cell_ in enumerate(cells)}
    rows = np.array([row_of.get(int(v), -1) for v in out["vertex_cell"]])
    assert (rows >= 0).sum() > 0.5 * len(rows)
    distance = np.linalg.norm(source[rows >= 0] - got[rows[rows >= 0]], axis=1)
    print("%s factor %d: largest distance to the image %.6g m, bound %.6g" % (kind, factor, distance.max(), np.sqrt(3) * (c + tol)))
    assert (distance <= np.sqrt(3) * c + np.sqrt(3) * tol).all()
    # weights: the vertices of the emitted cells
    assert out["weight"][:kv].tolist() == [int((out["vertex_cell"] == cell_).sum()) for cell_ in cells]
    assert (out["weight"][kv:] == -1).all() and np.isnan(out["xyz"][kv:]).all() and (out["rgb"][kv:] == 0).all()
    normals = out["normal"][:kv].astype(np.float64)
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("kind", ["sphere", "box"])
@pytest.mark.parametrize("factor", [2, 4, 8])
def test_without_dedupe_a_closed_mesh_stays_a_closed_chain(kind, factor):
    _, mesh, out, _, _ = run(kind, factor, 0)
    kt = int(out["num"][5])
    assert out["num"][10] == 0 and out["num"][6] == kt == int(mesh["num"][0]) - out["num"][9]
    assert sref.balanced(out["tri"][:kt])


@pytest.mark.parametrize("kind", ["sphere", "box"])
@pytest.mark.parametrize("factor", [2, 4, 8])
def test_with_dedupe_triangles_are_distinct_and_counts_add_up(kind, factor):
    _, mesh, out, _, _ = run(kind, factor, 1)
    kv, kt = int(out["num"][0]), int(out["num"][5])
    tri = out["tri"][:kt]
    assert (tri >= 0).all() and (tri < kv).all() and out["num"][7] == 0
    assert all(len({a, b, c}) == 3 for a, b, c in tri.tolist())                        # no triangle repeats a vertex
    assert (tri[:, 0] < tri[:, 1]).all() and (tri[:, 0] < tri[:, 2]).all()              # the canonical rotation
    assert len({tuple(t) for t in tri.tolist()}) == kt                                  # no two equal as oriented triples
    assert set(tri.reshape(-1).tolist()) == set(range(kv))                              # every vertex is referenced
    assert (np.diff(out["source"]) > 0).all()
    assert out["num"][6] + out["num"][9] + out["num"][10] + out["num"][11] == mesh["num"][0]
    without = run(kind, factor, 0)[2]
    assert out["num"][6] + out["num"][10] == without["num"][6] and np.array_equal(out["cells"], without["cells"])


@pytest.mark.parametrize("kind", ["sphere", "box"])
def test_factors_shrink_the_mesh_monotonically(kind):
    _, mesh, _, _, _ = run(kind, 2, 1)
    counts = [int(mesh["num"][0])] + [int(run(kind, factor, 1)[2]["num"][5]) for factor in (2, 4, 8)]
    vertices = [int(mesh["surface"]["num"][0])] + [int(run(kind, factor, 1)[2]["num"][0]) for factor in (2, 4, 8)]
    print(kind, "triangles", counts, "vertices", vertices)
    assert all(a > b > 0 for a, b in zip(counts, counts[1:])) and all(a > b > 0 for a, b in zip(vertices, vertices[1:]))


def test_capacities_in_the_restatement():
    _, _, full, _, _ = run("sphere", 4, 1)
    kv, kt = int(full["num"][1]), int(full["num"][6])
    few = run("sphere", 4, 1, max_vertices=kv // 2, max_triangles=kt // 2)[2]
    lost = (full["tri"][:kt // 2] >= kv // 2).any(axis=1)
    assert few["num"].tolist()[:3] == [kv // 2, kv, 1] and few["num"].tolist()[5:9] == [kt // 2, kt, int(lost.sum()), 1]
    assert 0 < lost.sum() < kt // 2 and (few["tri"][:kt // 2][lost] == -1).all()
    assert np.array_equal(few["tri"][:kt // 2][~lost], full["tri"][:kt // 2][~lost])
    assert few["xyz"].tobytes() == full["xyz"][:kv // 2].tobytes()


def test_the_home_slot_and_sizes_of_the_library():
    from regnet_for_3d_grasping_amd import _lib
    from regnet_for_3d_grasping_amd.csrc import build
    L = _lib.lib
    assert dict(build.SOURCES)["mesh_simplify.hip"] == ["-ffp-contract=off"] and build.NO_VGPR_SPILL["mesh_simplify.o"] == ["ms_"]
    assert L.regnet_mesh_simplify_table_slots(1) == 2 and L.regnet_mesh_simplify_table_slots(1000) == 2048
    assert L.regnet_mesh_simplify_table_slots(1 << 22) == 1 << 23 and L.regnet_mesh_simplify_table_slots((1 << 22) + 1) == -1
    for key in (0, 1, (5 << 42) | (9 << 21) | 11, (1 << 63) - 1):
        for slots in (2, 2048, 1 << 22, 1 << 23):
            want = ((key * 0x9E3779B97F4A7C15) % (1 << 64)) >> (64 - (slots.bit_length() - 1))
            assert L.regnet_mesh_simplify_home_slot_host(key, slots) == want
            if slots <= 1 << 22:                            # (the fusion's table ends there)
                assert L.regnet_fuse_home_slot_host(key, slots) == want
    assert L.regnet_mesh_simplify_home_slot_host(1, 3) == -1 and L.regnet_mesh_simplify_home_slot_host(1, 1 << 24) == -1
    assert L.regnet_mesh_simplify_workspace_bytes(0, 8) == -1 and L.regnet_mesh_simplify_workspace_bytes((1 << 21) + 1, 8) == -1
    assert L.regnet_mesh_simplify_workspace_bytes(8, (1 << 22) + 1) == -1
    small, large = L.regnet_mesh_simplify_workspace_bytes(1, 1), L.regnet_mesh_simplify_workspace_bytes(1 << 21, 1 << 22)
    assert 0 < small < 1024 and small % 16 == 0 and 84 << 21 < large < 1 << 29
